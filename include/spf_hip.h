/*
 * spf_hip.h — C ABI of the MI355X (gfx950) bootstrap engine.
 *
 * Drop-in boundary for the programmable-bootstrap hot path of Sunscreen-tech/spf.  The
 * reference has no FFI of its own; its seam is the concrete struct
 * `parasol_runtime::Evaluation` (parasol_runtime/src/crypto/evaluation.rs:144-266), whose
 * methods take caller-allocated `&mut` outputs, never fail, and are called concurrently from
 * rayon workers (circuit_processor/mod.rs:201-209).  Every entry point below names the
 * reference method / function whose body it replaces.  Citations are relative to the
 * reference repository root.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every call returns spf_status (0 = OK) and
 *     leaves a message retrievable with spf_last_error().
 *   - all arrays are dense, row-major, little-endian, in the reference's own layouts:
 *       LWE(n)        n mask words then the body                     entities/lwe_ciphertext.rs:24-33
 *       GLWE(k,N)     k mask polynomials then the body polynomial    entities/glwe_ciphertext.rs:32-41
 *       GGSW-FFT      [row<k+1][level<l][poly<k+1][bin<N/2]{re,im}   entities/ggsw_ciphertext_fft.rs:23-29
 *       BSK-FFT       [i<n] GGSW-FFT, natural DFT bin order           entities/bootstrap_key.rs:119-125
 *       KSK           [i<k*N][level<l_ks][n+1]                        entities/lwe_keyswitch_key.rs:27-36
 *     Torus elements are uint64_t (Torus<u64>, math/torus.rs:213); complex bins are
 *     interleaved {double re, double im} (num_complex::Complex<f64>).
 *   - "_batch" entry points take HOST pointers (what a Rust shim holding `&[u64]` passes) and
 *     stage through device memory; "_dev" entry points take DEVICE pointers plus a hipStream_t
 *     (passed as void*) and are asynchronous on that stream.  A "_batch" call returns only after
 *     the device is done with the caller's buffers, on failure as well as on success.
 *   - a context is bound to one GPU.  Calls on one context are serialised internally (thread-safe); use one context per
 *     stream for concurrency.  A device group (spf_group_*) holds one context per GPU of the node for ONE host process.
 */
#ifndef SPF_HIP_H
#define SPF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int spf_status;
enum {
    SPF_OK = 0,
    SPF_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, size mismatch, unsupported parameter */
    SPF_ERR_HIP = 2,              /* a HIP runtime call failed (message has the HIP error) */
    SPF_ERR_NO_KEY = 3,           /* the key this operation needs has not been loaded */
    SPF_ERR_UNSUPPORTED = 4       /* parameter set outside what the kernels are built for */
};

/* Mirror of `parasol_runtime::Params` (parasol_runtime/src/params.rs:10-100; DEFAULT_128 at
 * :107-134) restricted to the fields the bootstrap / keyswitch path reads. */
typedef struct spf_params {
    uint32_t lwe_dimension;     /* l0_params.dim            = 637  */
    uint32_t polynomial_degree; /* l1_params.dim.polynomial_degree = 2048 */
    uint32_t glwe_size;         /* l1_params.dim.size       = 1    */
    uint32_t pbs_radix_log;     /* pbs_radix.radix_log      = 16   */
    uint32_t pbs_radix_count;   /* pbs_radix.count          = 2    */
    uint32_t cbs_radix_log;     /* cbs_radix.radix_log      = 4    */
    uint32_t cbs_radix_count;   /* cbs_radix.count          = 4    */
    uint32_t ks_radix_log;      /* ks_radix.radix_log       = 2    */
    uint32_t ks_radix_count;    /* ks_radix.count           = 6    */
    uint32_t tr_radix_log;      /* tr_radix.radix_log       = 7    (trace / automorphism keyswitch) */
    uint32_t tr_radix_count;    /* tr_radix.count           = 6    */
    uint32_t ss_radix_log;      /* ss_radix.radix_log       = 3    (scheme switch) */
    uint32_t ss_radix_count;    /* ss_radix.count           = 15   */
} spf_params;

/* DEFAULT_128 (parasol_runtime/src/params.rs:107-134): the parameter set the tuned kernels are built for (lwe_dimension and the
 * keyswitch radix are free).  Any other set with polynomial_degree a power of two in 16 .. 2048 and radices with
 * radix_log * count < 64 whose (glwe_size + 1) polynomials fit one CU's LDS is served by a generic, untuned kernel family with the
 * same results as the reference's generic functions (every entry point: batch and device-pointer forms, the pool by host pointer
 * and by handle, the gate graphs, the device group); anything else — e.g. polynomial_degree 2048 with glwe_size >= 2 — is
 * SPF_ERR_UNSUPPORTED. */
void spf_default_params(spf_params *out);

typedef struct spf_ctx spf_ctx;

/* Replaces `Evaluation::new` (crypto/evaluation.rs:161-197) minus key ownership: creates the
 * per-GPU engine (twiddle tables, scratch).  device_id is the HIP ordinal. */
spf_status spf_create(const spf_params *params, int device_id, spf_ctx **out);
void spf_destroy(spf_ctx *ctx);
/* Lifetimes.  A child keeps its parent alive, and the destroy functions may be called in ANY order, each exactly once per
 * handle.  spf_graph_create and spf_pool_create retain their context; spf_graph_destroy and spf_pool_destroy release it.
 * spf_destroy drops the caller's reference: the context's streams and device memory go with the last one, and graphs and
 * pools made from the context stay fully usable (run, submit, wait, download) until they are destroyed themselves.
 * spf_group_graph_create and spf_pool_create_group retain the group; the group holds one reference on each member context and
 * a merged graph one on its member's.  spf_group_destroy drops the caller's reference: the communicators, the member threads,
 * the merged graphs and the group's references on its members go with the last one, so after it a job can still be read
 * (spf_graph_member, spf_graph_stats), run and destroyed, and a group pool — or a pool or graph made on a context borrowed
 * through spf_group_ctx — goes on working.  Values keep their own rule (below: they may outlive their pool, and are refused,
 * never trusted, by any other pool).
 * The caller's duty, NOT detected by the library: no use of a handle after its own destroy (that includes passing the
 * spf_ctx* to any call after spf_destroy, and the spf_group* after spf_group_destroy); no second destroy of a handle; no
 * destroy while another thread is inside a call on that handle; no spf_destroy on a context borrowed through spf_group_ctx;
 * no spf_device_free after the context's last reference is gone. */

/* Process-wide counts of the handles that exist: made and not yet freed (a context or group that its children keep alive
 * still counts; a group pool counts itself and one pool per member; a group's merged graphs count as graphs).  Atomic
 * counters moved in the constructors and at the final frees: how a host without a leak checker sees a lost reference. */
typedef struct spf_live_counts {
    uint64_t contexts, groups, graphs, pools, values;
} spf_live_counts;
spf_status spf_live_objects(spf_live_counts *out);
/* Message of the last failing call on this context (or, with ctx == NULL, of the last failing
 * spf_create on the calling thread).  The returned pointer is storage of the calling thread: it
 * stays valid until that thread calls spf_last_error again, whatever other threads do. */
const char *spf_last_error(const spf_ctx *ctx);

/* ---- keys: `ComputeKey` fields (crypto/keys.rs:306-318) ------------------------------- */

/* `ComputeKey::bs_key` : BootstrapKeyFft<Complex<f64>>.  n_complex must equal
 * lwe_dimension * (k+1)*l_pbs*(k+1)*N/2.  Host pointer; copied to HBM.  The engine also keeps a copy
 * scaled by 2^-10 for its blind-rotation kernels (the inverse transform's 1/N travels with the key: exact
 * for every spectrum a torus polynomial has, results unchanged), so a key holding a NaN or a non-zero
 * magnitude outside [2^-900, 2^1000) — which no forward transform produces — is refused with
 * SPF_ERR_INVALID_ARGUMENT here and in spf_key_blob_commit(ctx, 0), and leaves the context without a
 * bootstrap key. */
spf_status spf_load_bootstrap_key(spf_ctx *ctx, const double *bsk_fft, size_t n_complex);
/* `ComputeKey::ks_key` : LweKeyswitchKey<u64>.  n_words = k*N * l_ks * (lwe_dimension+1). */
spf_status spf_load_keyswitch_key(spf_ctx *ctx, const uint64_t *ksk, size_t n_words);

/* `ComputeKey::auto_key` : AutomorphismKeyFft<Complex<f64>> = log2(N) GLWE keyswitch keys
 * [i<log2 N][row<k][level<l_tr][poly<k+1][bin<N/2] (entities/automorphism_key.rs). */
spf_status spf_load_automorphism_key(spf_ctx *ctx, const double *ak_fft, size_t n_complex);
/* `ComputeKey::ss_key` : SchemeSwitchKeyFft<Complex<f64>> = k(k+1)/2 GLEVs
 * [pair][level<l_ss][poly<k+1][bin<N/2] (entities/scheme_switch_key.rs). */
spf_status spf_load_scheme_switch_key(spf_ctx *ctx, const double *ssk_fft, size_t n_complex);

/* ---- keys in standard (integer) form: `ComputeKeyNonFft` fields (crypto/keys.rs:145-159) -----------------------------
 * The reference's portable key form is the integer one: `ComputeKeyNonFft` is what it serializes, and `ComputeKeyNonFft::fft`
 * (keys.rs:258-282) makes the `ComputeKey` above from it; the float form "can be represented with insufficient precision" in
 * transit (keys.rs:294-305).  "Standard form" = Torus<u64> words in the reference's layouts `BootstrapKey<u64>`,
 * `AutomorphismKey<u64>`, `SchemeSwitchKey<u64>`: the FFT layouts above with every block of N/2 complex bins replaced by the
 * polynomial's N words — the reference's `.fft()` is a flat map over the polynomials in storage order
 * (entities/bootstrap_key.rs:92-105 -> ggsw_ciphertext.rs:98 -> glev_ciphertext.rs:66 -> glwe_ciphertext.rs:141;
 * automorphism_key.rs:68 -> glwe_keyswitch_key.rs:80; scheme_switch_key.rs:174), each `PolynomialRef::fft`
 * (entities/polynomial.rs:257-274).  Handing keys over this way, the library's own forward transform is the
 * only floating-point step a key goes through: results do not depend on the host's FFT.
 *
 * `spf_poly_fft_*`: B x `PolynomialRef::fft` — n_polys x N words in, n_polys x N/2 complex bins out, each word taken as
 * (double)(int64_t)w; bit-equal to the oracle's transform.  Also what brings an integer-form GGSW / GLEV / GLWE ciphertext into the
 * transform domain (`GgswCiphertext::fft` & co. above).  A polynomial and its spectrum have the same size: in the `_dev` form
 * d_out == d_in (in place) is allowed; any other overlap is SPF_ERR_INVALID_ARGUMENT.  n_polys = 0 is SPF_OK. */
spf_status spf_poly_fft_dev(spf_ctx *ctx, void *stream, size_t n_polys, const uint64_t *d_in, double *d_out);
spf_status spf_poly_fft_batch(spf_ctx *ctx, size_t n_polys, const uint64_t *in, double *out);
/* `BootstrapKey::fft` (entities/bootstrap_key.rs:92-105) / `fft_bootstrap_key` + upload: n_words = 2 x the n_complex of
 * spf_load_bootstrap_key.  The length is checked before the device is touched; the words are copied into the key blob and
 * transformed there (no second buffer), then the key is finished as spf_load_bootstrap_key finishes it.  On any failure the
 * context is left without that key. */
spf_status spf_load_bootstrap_key_std(spf_ctx *ctx, const uint64_t *bsk, size_t n_words);
/* `AutomorphismKey::fft` (entities/automorphism_key.rs:68): n_words = 2 x the n_complex of spf_load_automorphism_key */
spf_status spf_load_automorphism_key_std(spf_ctx *ctx, const uint64_t *ak, size_t n_words);
/* `SchemeSwitchKey::fft` (entities/scheme_switch_key.rs:174): n_words = 2 x the n_complex of spf_load_scheme_switch_key */
spf_status spf_load_scheme_switch_key_std(spf_ctx *ctx, const uint64_t *ssk, size_t n_words);
/* The key of spf_public_functional_keyswitch_* below: `PublicFunctionalKeyswitchKey<u64>`
 * (sunscreen_tfhe/src/entities/public_functional_keyswitch_key.rs), [from_dimension][radix_count][k+1][N] words — row (i, lvl) is a
 * GLWE.  Integer form only, like the other `_std` loaders: the words are copied into a key blob and transformed there by the
 * library's own forward transform (no host FFT, no float loader).  The radix belongs to the KEY, not to spf_params.
 * n_words = from_dimension * radix_count * (k+1) * N; from_dimension >= 1, radix_log >= 1, radix_count >= 1,
 * radix_log * radix_count < 64 and from_dimension * radix_count <= 0x0fffffff, else SPF_ERR_INVALID_ARGUMENT; every check runs
 * before the device is touched.  On any failure the context is left without this key.  A reload with another from_dimension or
 * radix replaces the key. */
spf_status spf_load_public_functional_keyswitch_key_std(spf_ctx *ctx, const uint64_t *key, size_t n_words, size_t from_dimension,
                                                        uint32_t radix_log, uint32_t radix_count);
/* The keys of spf_private_functional_keyswitch_* below: n_keys x `PrivateFunctionalKeyswitchKey<u64>`
 * (sunscreen_tfhe/src/entities/private_functional_keyswitch_key.rs:44-46), back to back, each [lwe_count][from_dimension+1][radix_count][k+1][N]
 * words — row (z, i, lvl) is a GLWE; row i = from_dimension meets the body word.  `CircuitBootstrappingKeyswitchKeys<u64>`
 * (entities/circuit_bootstrapping_private_keyswitch_keys.rs:28-35) is n_keys = k+1, lwe_count = 1, from_dimension = k*N.  Integer form
 * only (the operation is integer arithmetic: nothing is transformed).  The radix belongs to the KEYS, not to spf_params.
 * n_words = n_keys * lwe_count * (from_dimension+1) * radix_count * (k+1) * N; n_keys, from_dimension, lwe_count >= 1, radix_log >= 1,
 * radix_count >= 1, radix_log * radix_count < 64, n_keys <= 65535, 8 * n_keys * (k+1) * N <= 0x7fffff00 and
 * lwe_count * (from_dimension+1) * radix_count <= 0x7fffff00, else SPF_ERR_INVALID_ARGUMENT; every check runs before the device is
 * touched.  On any failure the context is left without these keys.  A reload with another shape or radix replaces them. */
spf_status spf_load_private_functional_keyswitch_keys_std(spf_ctx *ctx, const uint64_t *keys, size_t n_words, size_t n_keys,
                                                          size_t from_dimension, size_t lwe_count, uint32_t radix_log,
                                                          uint32_t radix_count);

/* Multi-GPU key replication (no reference counterpart): the device-resident
 * key blobs, so that a caller can RCCL-broadcast rank 0's keys into every other rank's
 * context.  which: 0 = bootstrap key, 1 = keyswitch key, 2 = automorphism key,
 * 3 = scheme-switch key, 4 = public functional keyswitch key, 5 = private functional keyswitch keys (the words as loaded; 4 and 5
 * once their shape is known from a load on this context or, in a group, on member 0; before that SPF_ERR_NO_KEY).  Allocates the
 * blob if needed;
 * after filling it externally call spf_key_blob_commit. */
spf_status spf_key_blob(spf_ctx *ctx, int which, void **dev_ptr, size_t *bytes);
spf_status spf_key_blob_commit(spf_ctx *ctx, int which);

/* ---- the hot path, host-pointer batch forms --------------------------------------------- */

/* B x `Evaluation::keyswitch_lwe_l1_lwe_l0` (crypto/evaluation.rs:246-255) =
 * `keyswitch_lwe_to_lwe` (sunscreen_tfhe/src/ops/keyswitch/lwe_keyswitch.rs:23-62).
 * lwe1_in: B x (k*N+1), lwe0_out: B x (lwe_dimension+1). */
spf_status spf_keyswitch_lwe_l1_lwe_l0_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe1_in,
                                             uint64_t *lwe0_out);

/* B x `generalized_programmable_bootstrap`
 * (sunscreen_tfhe/src/ops/bootstrapping/programmable_bootstrapping.rs:342-410).
 * lwe0_in : B x (lwe_dimension+1)
 * lut_glwe: the UnivariateLookupTable's GLWE, (k+1)*N words; lut_stride = 0 shares one LUT
 *           across the batch, otherwise ciphertext j uses lut_glwe + j*lut_stride.
 * body_rotate is added to each input body first (`lwe_rotate`,
 *           ops/homomorphisms/lwe.rs:9-20; 0 for a plain PBS).
 * glwe_out: B x (k+1)*N. */
spf_status spf_generalized_pbs_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe0_in,
                                     const uint64_t *lut_glwe, size_t lut_stride, uint32_t log_chi,
                                     uint32_t log_v, uint64_t body_rotate, uint64_t *glwe_out);

/* B x `programmable_bootstrap_univariate` (programmable_bootstrapping.rs:291-318):
 * generalized PBS with (log_chi, log_v) = (0, 0) then `sample_extract(., 0)`.
 * lwe1_out: B x (k*N+1). */
spf_status spf_pbs_univariate_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe0_in,
                                    const uint64_t *lut_glwe, size_t lut_stride,
                                    uint64_t *lwe1_out);

/* B x `programmable_bootstrap_bivariate` (programmable_bootstrapping.rs:575-621): packs
 * left * 2^plaintext_bits + right on every word, wrapping (`scalar_mul_ciphertext_mad` into a cleared LWE, then
 * `add_lwe_inplace`, :603-610), then bootstraps the packed input as spf_pbs_univariate_batch does; word-equal to
 * spf_pbs_univariate_batch of the packed batch.  lwe0_left, lwe0_right: B x (lwe_dimension+1) each (they may be the
 * same array: f(x, x)); lut_glwe / lut_stride as above, typically from spf_generate_bivariate_lut.  Encoding the inputs
 * (padding bit, carry room) is the caller's.  plaintext_bits >= 64 is SPF_ERR_INVALID_ARGUMENT.
 * lwe1_out: B x (k*N+1). */
spf_status spf_pbs_bivariate_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe0_left, const uint64_t *lwe0_right,
                                   const uint64_t *lut_glwe, size_t lut_stride, uint32_t plaintext_bits,
                                   uint64_t *lwe1_out);

/* B x the bootstrap stage of `Evaluation::circuit_bootstrap` (crypto/evaluation.rs:211-226):
 * `hi_noise_lwe_to_lo_noise_glwe` (ops/bootstrapping/circuit_bootstrapping.rs:387-427) =
 * rotate by q/4, multifunctional CBS LUT (:430-482), generalized PBS with
 * log_v = ceil(log2(cbs_radix_count)).  glwe_out: B x (k+1)*N. */
spf_status spf_circuit_bootstrap_pbs_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe0_in,
                                           uint64_t *glwe_out);

/* B x `Evaluation::circuit_bootstrap` (crypto/evaluation.rs:211-226) =
 * `circuit_bootstrap_via_trace_and_scheme_switch` (ops/bootstrapping/circuit_bootstrapping.rs:342-385):
 * the bootstrap above, then `mod_switch_trace_and_rotate` (:260-298) and `scheme_switch_fft`
 * (ops/fft_ops.rs:403-442).  ggsw_fft_out: B x (k+1)*l_cbs*(k+1)*N/2 complex, the layout
 * `L1GgswCiphertext` holds and `cmux` consumes.  Needs all four keys. */
spf_status spf_circuit_bootstrap_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe0_in,
                                       double *ggsw_fft_out);
/* B x `mod_switch_trace_and_rotate` alone: lo-noise GLWE -> GLEV (l_cbs GLWEs per ciphertext). */
spf_status spf_mod_switch_trace_and_rotate_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in,
                                                 uint64_t *glev_out);
/* B x `Evaluation::scheme_switch` (crypto/evaluation.rs:231-240) = `scheme_switch_fft`:
 * GLEV (l_cbs GLWEs) -> GGSW-FFT. */
spf_status spf_scheme_switch_batch(spf_ctx *ctx, size_t B, const uint64_t *glev_in, double *ggsw_fft_out);

/* B x `KeylessEvaluation::sample_extract_l1` (crypto/evaluation.rs:126-133) =
 * `sample_extract` (ops/ciphertext/glwe_ciphertext_ops.rs:31-76), same index for the batch. */
spf_status spf_sample_extract_l1_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in, size_t idx,
                                       uint64_t *lwe1_out);

/* The linear `KeylessEvaluation` operations on L1 GLWE ciphertexts (B x (k+1)*N words each):
 *   not    (crypto/evaluation.rs:47-50): out = in + trivial_one, i.e. body coefficient 0 += 2^63
 *          (`trivial_glwe_l1_one`, crypto/encryption.rs:359-364, one plaintext bit :132);
 *   xor    (:52-55): out = a + b, wrapping;
 *   mul_xn (:57-65): out = in * X^n mod X^N + 1 = `rotate_glwe_positive_monomial_negacyclic`
 *          (sunscreen_tfhe/src/ops/bootstrapping/blind_rotation.rs:126-135), same n for the batch,
 *          n taken mod 2N (entities/polynomial.rs:208-236). */
spf_status spf_glwe_not_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
spf_status spf_glwe_xor_batch(spf_ctx *ctx, size_t B, const uint64_t *a, const uint64_t *b,
                              uint64_t *glwe_out);
spf_status spf_glwe_mul_xn_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in, size_t n,
                                 uint64_t *glwe_out);

/* B x `KeylessEvaluation::cmux` (crypto/evaluation.rs:68-83) = `cmux`
 * (sunscreen_tfhe/src/ops/fft_ops.rs:149-181) with the GGSW in cbs_radix shape.
 * sel_ggsw_fft: B x (k+1)*l_cbs*(k+1)*N/2 complex; a (selected when 0), b (when 1), out:
 * B x (k+1)*N. */
spf_status spf_cmux_batch(spf_ctx *ctx, size_t B, const double *sel_ggsw_fft, const uint64_t *a,
                          const uint64_t *b, uint64_t *out);

/* B x `KeylessEvaluation::glev_cmux` (crypto/evaluation.rs:86-101) = `glev_cmux`
 * (ops/fft_ops.rs:203-220): one selector per item; a / b / out are GLEVs of l_cbs GLWEs
 * (B x l_cbs x (k+1)*N words). */
spf_status spf_glev_cmux_batch(spf_ctx *ctx, size_t B, const double *sel_ggsw_fft, const uint64_t *a,
                               const uint64_t *b, uint64_t *out);
/* B x `KeylessEvaluation::multiply_glwe_ggsw` (crypto/evaluation.rs:104-123):
 * out = IFFT(glwe [*] ggsw), `glwe_ggsw_mad` into a cleared accumulator (ops/fft_ops.rs:23-56). */
spf_status spf_multiply_glwe_ggsw_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe, const double *ggsw_fft,
                                        uint64_t *out);

/* The north-star "gate": keyswitch L1->L0 then the circuit-bootstrap PBS, fused on device
 * (FheOp::KeyswitchL1toL0 -> FheOp::CircuitBootstrap, circuit_processor/mod.rs:329-340,453-463).
 * lwe1_in: B x (k*N+1); glwe_out: B x (k+1)*N. */
spf_status spf_gate_bootstrap_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe1_in,
                                    uint64_t *glwe_out);
/* B x (FheOp::KeyswitchL1toL0 -> FheOp::CircuitBootstrap) with the whole circuit bootstrap
 * (`Evaluation::keyswitch_lwe_l1_lwe_l0` then `Evaluation::circuit_bootstrap`, crypto/evaluation.rs:211-266):
 * L1 LWE in, L1 GGSW-FFT out (cbs radix); the level-0 LWE in between stays in HBM. */
spf_status spf_keyswitch_circuit_bootstrap_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe1_in,
                                                 double *ggsw_fft_out);

/* Packed integers (`PackedDynamicGenericInt`, parasol_runtime fluent/generic_int.rs:162-176): an n_bits-bit integer in ONE
 * L1 GLWE, bit i (least significant first, fluent/int.rs:47-49, uint.rs:30-32) in coefficient X^i.  Every entry point below is
 * int-major: bit i of packed ciphertext b is row b * n_bits + i.  0 < n_bits <= N (dynamic_generic_int_graph_nodes.rs:146-147)
 * and B * n_bits <= 0x0fffffff, else SPF_ERR_INVALID_ARGUMENT before any device work; B = 0 is SPF_OK.  Pack and
 * unpack need no key.
 * glwe_pack: `DynamicGenericIntGraphNodes::pack` (fluent/dynamic_generic_int_graph_nodes.rs:139-200) = sum over i of
 *   `MulXN(i)` of bit i's GLWE, one kernel; word-equal to the reference's tree of `GlweAdd`s (addition mod 2^64 is
 *   associative).  bits_glwe: B * n_bits x (k+1)*N; packed_out: B x (k+1)*N.
 * glwe_unpack_l1: `PackedDynamicGenericIntGraphNode::unpack` (fluent/packed_dynamic_generic_int_graph_node.rs:24-39) =
 *   `SampleExtract(i)` for i < n_bits, one kernel.  packed_glwe: B x (k+1)*N; lwe1_out: B * n_bits x (k*N+1).
 * unpack_circuit_bootstrap: the unpack, then `KeyswitchL1toL0` -> `CircuitBootstrap` of every bit (fhe_circuit.rs:563-625);
 *   the L1 and L0 LWEs stay on the device.  Bit-equal to spf_keyswitch_circuit_bootstrap_batch of the unpacked LWEs, and
 *   fails as it does without a key or with an unsupported circuit-bootstrap tail.  ggsw_fft_out: B * n_bits GGSWs. */
spf_status spf_glwe_pack_batch(spf_ctx *ctx, size_t B, size_t n_bits, const uint64_t *bits_glwe, uint64_t *packed_out);
spf_status spf_glwe_unpack_l1_batch(spf_ctx *ctx, size_t B, size_t n_bits, const uint64_t *packed_glwe, uint64_t *lwe1_out);
spf_status spf_unpack_circuit_bootstrap_batch(spf_ctx *ctx, size_t B, size_t n_bits, const uint64_t *packed_glwe,
                                              double *ggsw_fft_out);

/* `blind_rotation` (sunscreen_tfhe/src/ops/bootstrapping/blind_rotation.rs:202-223): out = in * X^-(s << log_stride), the shift s
 * given as GGSW encryptions of its bits in cbs_radix shape (`BlindRotationShiftFft`, entities/blind_rotation_shift.rs), int-major
 * like the packed integers above: bit i (least significant first) of item b is selector b * n_bits + i — what
 * spf_unpack_circuit_bootstrap_* produces.  For i ascending, acc = `cmux`(shift[b][i], acc, X^-(2^(i + log_stride)) * acc)
 * (ops/fft_ops.rs:149-181; `rotate_glwe_negative_monomial_negacyclic`, blind_rotation.rs:107-116: coefficient j of the rotated
 * GLWE is coefficient j + r of the input, negated where j + r >= N), one kernel per bit whose high operand is a rotated read of
 * the low one.  Word-equal to the same loop of spf_glwe_mul_xn_batch (amount 2N - r) and spf_cmux_batch.  The reference's call
 * is n_bits = log2 N, log_stride = 0; log_stride indexes entries of 2^log_stride coefficients (a packed table).  No key.
 * shift_ggsw_fft: B * n_bits x (k+1)*l_cbs*(k+1)*N/2 complex; glwe_in, glwe_out: B x (k+1)*N.
 * n_bits >= 1, n_bits + log_stride <= log2 N and B * n_bits <= 0x0fffffff, else SPF_ERR_INVALID_ARGUMENT before any device
 * work; B = 0 is SPF_OK; a tuned context whose cbs radix is not 4 x 4 bits: SPF_ERR_UNSUPPORTED, as for spf_cmux_batch. */
spf_status spf_blind_rotation_batch(spf_ctx *ctx, size_t B, size_t n_bits, size_t log_stride, const double *shift_ggsw_fft,
                                    const uint64_t *glwe_in, uint64_t *glwe_out);

/* `public_functional_keyswitch` (sunscreen_tfhe/src/ops/keyswitch/public_functional_keyswitch.rs:74-148; its leg of the
 * reference's benchmark: benches/ops.rs:395-452) with the public map of the reference's test and benchmark, message j to
 * coefficient j: lwe_count <= N LWE ciphertexts (a_j, b_j) of dimension from_dimension in, ONE GLWE out whose coefficient j holds
 * message j — an LWE enters GLWE-land without a bootstrap.  poly_i = sum_j a_j[i] X^j; for i ascending
 * `decomposed_polynomial_glev_mad`(acc_fft, Decomp(poly_i), fft(K[i])) (ops/fft_ops.rs:67-98) into ONE spectrum; out = -(ifft(acc_fft))
 * on every polynomial, then out.body[j] += b_j.  Rows ascending, digits as the reference has them, one inverse transform: the
 * order is part of the function.  Key: spf_load_public_functional_keyswitch_key_std.
 * lwe_in: B * lwe_count rows of from_dimension + 1 words, int-major as in the packed calls (input j of output b is row
 * b * lwe_count + j); glwe_out: B x (k+1)*N.  No key: SPF_ERR_NO_KEY.  lwe_count = 0, lwe_count > N, B * lwe_count > 0x0fffffff
 * or a null pointer: SPF_ERR_INVALID_ARGUMENT before any device work.  B = 0 is SPF_OK. */
spf_status spf_public_functional_keyswitch_batch(spf_ctx *ctx, size_t B, size_t lwe_count, const uint64_t *lwe_in,
                                                 uint64_t *glwe_out);

/* `private_functional_keyswitch` (sunscreen_tfhe/src/ops/keyswitch/private_functional_keyswitch.rs:107-142): lwe_count LWE
 * ciphertexts ct_z = (a_z, b_z) of dimension n = from_dimension in, ONE GLWE out, under the secret linear map baked into key
 * `key_index` of the loaded set:  out = - sum_z sum_{i <= n} sum_j digit_j(ct_z[i]) * K[z][i][count-1-j], every word mod 2^64
 * (`ScalarRadixIterator` digits, math/radix.rs; GLEV levels in reverse, `decomposed_scalar_glev_mad`, glev_ciphertext_ops.rs:48-59;
 * the body word is row i = n and is decomposed like the mask words; no body is added afterwards).  Integer arithmetic only: the
 * words are the reference's, bit for bit.  Keys: spf_load_private_functional_keyswitch_keys_std.
 * lwe_in: B * lwe_count rows of from_dimension + 1 words (input z of output b is row b * lwe_count + z); glwe_out: B x (k+1)*N.
 * No keys: SPF_ERR_NO_KEY.  key_index >= n_keys, B > 0x0fffffff or a null pointer: SPF_ERR_INVALID_ARGUMENT before any device
 * work.  B = 0 is SPF_OK. */
spf_status spf_private_functional_keyswitch_batch(spf_ctx *ctx, size_t key_index, size_t B, const uint64_t *lwe_in,
                                                  uint64_t *glwe_out);
/* `apply_pfks_on_ggsw_components` (ops/bootstrapping/circuit_bootstrapping.rs:485-514): GGSW row (r, level) is the private
 * functional keyswitch of LWE `level` under key r.  lwe_in: B * l_cbs rows of k*N + 1 words; ggsw_out: B INTEGER-form GGSWs in the
 * reference's layout [k+1][l_cbs][k+1][N].  Needs n_keys = k+1, lwe_count = 1, from_dimension = k*N, else
 * SPF_ERR_INVALID_ARGUMENT.  One launch sequence (the digits of a row are computed once and meet all k+1 keys), word-equal to
 * k+1 calls of the single operation placed by hand. */
spf_status spf_apply_pfks_on_ggsw_components_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe_in, uint64_t *ggsw_out);
/* `circuit_bootstrap_via_pfks` (ops/bootstrapping/circuit_bootstrapping.rs:162-219; its leg of the reference's benchmark:
 * benches/ops.rs:172-234): `hi_noise_lwe_to_lo_noise_glwe` (what spf_circuit_bootstrap_pbs_* computes), then
 * `extract_and_rotate_lo_noise_glwe` (:224-252: `sample_extract`(i) and 2^(64 - (cbs_radix_log*(i+1) + 1)) onto the body, i < l_cbs),
 * then the components call above, then the library's forward transform on every polynomial (spf_poly_fft_*).
 * ggsw_fft_out: B x (k+1)*l_cbs*(k+1)*N/2 complex, the layout spf_cmux_* consumes.  Needs the bootstrap key and a key set of the
 * components call's shape. */
spf_status spf_circuit_bootstrap_via_pfks_batch(spf_ctx *ctx, size_t B, const uint64_t *lwe0_in, double *ggsw_fft_out);

/* ---- device-pointer forms (inputs/outputs resident in HBM, asynchronous on `stream`) -----
 * Contract of every `_dev` entry point: the call only ENQUEUES on `stream`; inputs and outputs must stay valid and
 * unchanged until that work has completed; an output must not overlap any input of the same call.  The entry points that
 * need intermediates (`spf_circuit_bootstrap_dev`, the keyswitch, `spf_pbs_bivariate_dev`'s packed input,
 * `spf_blind_rotation_dev`'s accumulator between steps) keep them in
 * buffers of the CONTEXT: enqueue them on ONE stream per context (or order the streams with events) — two such calls
 * running concurrently on different streams would share those buffers.  A call that has to grow a buffer of the context (a
 * larger batch than the context has seen) may wait for the device before it returns.  `spf_mod_switch_trace_and_rotate_dev`
 * additionally uses its OUTPUT as working memory while it runs (the kernel parks half of its accumulator in each unit's
 * 32 KiB of `d_glev_out` between automorphism rounds):
 * `d_glev_out` holds intermediate data until the kernel has completed and must not be read, or alias anything read, by
 * work that may run concurrently with it. */

spf_status spf_keyswitch_lwe_l1_lwe_l0_dev(spf_ctx *ctx, void *stream, size_t B,
                                           const uint64_t *d_lwe1_in, uint64_t *d_lwe0_out);
spf_status spf_generalized_pbs_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_lwe0_in,
                                   const uint64_t *d_lut_glwe, size_t lut_stride, uint32_t log_chi,
                                   uint32_t log_v, uint64_t body_rotate, uint64_t *d_glwe_out);
spf_status spf_pbs_univariate_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_lwe0_in,
                                  const uint64_t *d_lut_glwe, size_t lut_stride,
                                  uint64_t *d_lwe1_out);
/* spf_pbs_bivariate_batch on device pointers: the packed input lives in a buffer of the context (one stream per context) */
spf_status spf_pbs_bivariate_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_lwe0_left,
                                 const uint64_t *d_lwe0_right, const uint64_t *d_lut_glwe, size_t lut_stride,
                                 uint32_t plaintext_bits, uint64_t *d_lwe1_out);
spf_status spf_circuit_bootstrap_pbs_dev(spf_ctx *ctx, void *stream, size_t B,
                                         const uint64_t *d_lwe0_in, uint64_t *d_glwe_out);
spf_status spf_circuit_bootstrap_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_lwe0_in,
                                     double *d_ggsw_fft_out);
spf_status spf_mod_switch_trace_and_rotate_dev(spf_ctx *ctx, void *stream, size_t B,
                                               const uint64_t *d_glwe_in, uint64_t *d_glev_out);
spf_status spf_scheme_switch_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_glev_in,
                                 double *d_ggsw_fft_out);
spf_status spf_sample_extract_l1_dev(spf_ctx *ctx, void *stream, size_t B,
                                     const uint64_t *d_glwe_in, size_t idx, uint64_t *d_lwe1_out);
spf_status spf_glwe_not_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_in, uint64_t *d_out);
spf_status spf_glwe_xor_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_a,
                            const uint64_t *d_b, uint64_t *d_out);
spf_status spf_glwe_mul_xn_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_in, size_t n,
                               uint64_t *d_out);
spf_status spf_cmux_dev(spf_ctx *ctx, void *stream, size_t B, const double *d_sel_ggsw_fft,
                        const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out);
spf_status spf_glev_cmux_dev(spf_ctx *ctx, void *stream, size_t B, const double *d_sel_ggsw_fft,
                             const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out);
spf_status spf_multiply_glwe_ggsw_dev(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_glwe,
                                      const double *d_ggsw_fft, uint64_t *d_out);
/* the packed-integer entry points on device pointers.  spf_glwe_pack_dev refuses an output range that overlaps the input
 * range; spf_unpack_circuit_bootstrap_dev keeps the unpacked LWEs in buffers of the context (one stream per context). */
spf_status spf_glwe_pack_dev(spf_ctx *ctx, void *stream, size_t B, size_t n_bits, const uint64_t *d_bits_glwe,
                             uint64_t *d_packed_out);
spf_status spf_glwe_unpack_l1_dev(spf_ctx *ctx, void *stream, size_t B, size_t n_bits, const uint64_t *d_packed_glwe,
                                  uint64_t *d_lwe1_out);
spf_status spf_unpack_circuit_bootstrap_dev(spf_ctx *ctx, void *stream, size_t B, size_t n_bits,
                                            const uint64_t *d_packed_glwe, double *d_ggsw_fft_out);

/* spf_blind_rotation_batch (`blind_rotation`, ops/bootstrapping/blind_rotation.rs:202-223) on device pointers.  With
 * n_bits > 1 the accumulator alternates between a B x GLWE buffer of the context (one stream per context) and d_glwe_out, the
 * last step writing d_glwe_out; d_glwe_in is only read.  An output range that overlaps an input range is refused. */
spf_status spf_blind_rotation_dev(spf_ctx *ctx, void *stream, size_t B, size_t n_bits, size_t log_stride,
                                  const double *d_shift_ggsw_fft, const uint64_t *d_glwe_in, uint64_t *d_glwe_out);

/* spf_public_functional_keyswitch_batch (`public_functional_keyswitch`, ops/keyswitch/public_functional_keyswitch.rs:74-148) on
 * device pointers, under the contract of the `_dev` entry points above: it only enqueues on `stream`; on a tuned context at radix
 * 4 bits x 8 or 4 x 4 the transposed digits of the inputs live in a buffer of the context (one stream per context), which grows
 * by the same rule.  An output range that overlaps the input range is refused. */
spf_status spf_public_functional_keyswitch_enqueue(spf_ctx *ctx, void *stream, size_t B, size_t lwe_count, const uint64_t *d_lwe_in,
                                                   uint64_t *d_glwe_out);

/* spf_private_functional_keyswitch_batch (`private_functional_keyswitch`, ops/keyswitch/private_functional_keyswitch.rs:107-142),
 * spf_apply_pfks_on_ggsw_components_batch (`apply_pfks_on_ggsw_components`, circuit_bootstrapping.rs:485-514) and
 * spf_circuit_bootstrap_via_pfks_batch (`circuit_bootstrap_via_pfks`, circuit_bootstrapping.rs:162-219) on device pointers, under
 * the contract of the `_dev` entry points above: each only enqueues on `stream`; the int8 limbs of the inputs and, for the circuit
 * bootstrap, the lo-noise GLWEs and the extracted rows live in buffers of the context (one stream per context), which grow by
 * the same rule.  An output range that overlaps the input range is refused. */
spf_status spf_private_functional_keyswitch_enqueue(spf_ctx *ctx, void *stream, size_t key_index, size_t B, const uint64_t *d_lwe_in,
                                                    uint64_t *d_glwe_out);
spf_status spf_apply_pfks_on_ggsw_components_enqueue(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_lwe_in,
                                                     uint64_t *d_ggsw_out);
spf_status spf_circuit_bootstrap_via_pfks_enqueue(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_lwe0_in,
                                                  double *d_ggsw_fft_out);

/* ciphertext types (`L0LweCiphertext` ... `L1GlevCiphertext`, crypto/encryption.rs:23-110) and the computing variants of `FheOp`
 * (fhe_circuit.rs:65-126): used by the values, the pool's generic submit and the gate graphs below */
typedef enum spf_value_kind {
    SPF_VAL_LWE0 = 0,  /* L0LweCiphertext: n+1 words */
    SPF_VAL_LWE1 = 1,  /* L1LweCiphertext: k*N+1 words */
    SPF_VAL_GLWE1 = 2, /* L1GlweCiphertext: (k+1)*N words */
    SPF_VAL_GGSW1 = 3, /* L1GgswCiphertext, FFT domain: (k+1)*l_cbs*(k+1)*N/2 complex */
    SPF_VAL_GLEV1 = 4  /* L1GlevCiphertext: l_cbs GLWEs */
} spf_value_kind;
typedef enum spf_graph_op {
    SPF_OP_SAMPLE_EXTRACT = 0,
    SPF_OP_KEYSWITCH_L1_TO_L0 = 1,
    SPF_OP_NOT = 2,
    SPF_OP_GLWE_ADD = 3,
    SPF_OP_CMUX = 4,
    SPF_OP_GLEV_CMUX = 5,
    SPF_OP_MULTIPLY_GGSW_GLWE = 6,
    SPF_OP_CIRCUIT_BOOTSTRAP = 7,
    SPF_OP_SCHEME_SWITCH = 8,
    SPF_OP_MUL_XN = 9,
    SPF_OP_PBS_UNIVARIATE = 10, /* no FheOp: `programmable_bootstrap_univariate` with the table as an operand (below) */
    SPF_OP_PBS_BIVARIATE = 11,  /* no FheOp: `programmable_bootstrap_bivariate`, param = plaintext_bits */
    /* no FheOp either: `keyswitch_glwe_to_glwe`, one round of the trace's loop and `trace` (spf_glwe_keyswitch_batch and its
     * neighbours below), one GLWE1 in, one GLWE1 out; param = the keyswitch-key slot (< SPF_GLWE_KSK_SLOTS) / the round
     * (1 .. log2 N) / ignored */
    SPF_OP_GLWE_KEYSWITCH = 12,
    SPF_OP_GLWE_AUTOMORPHISM = 13,
    SPF_OP_GLWE_TRACE = 14
} spf_graph_op;

/* ---- plaintext linear maps over LWE ciphertexts ---------------------------------------------
 * `scalar_mul_ciphertext_mad` then `add_lwe_inplace` (sunscreen_tfhe/src/ops/ciphertext/lwe_ciphertext_ops.rs:48-66, :4-18) — the
 * two calls `programmable_bootstrap_bivariate` makes for left * 2^bits + right — for any M x K matrix w of int64 weights and an
 * optional bias of M words:
 *   out[b][m][c] = sum_k (uint64_t)w[m][k] * in[b][k][c]   for every word c, mod 2^64;   out[b][m][W-1] += bias[m]
 * in [B][K][W], out [B][M][W]; the K ciphertexts are all SPF_VAL_LWE0 (W = n+1) or all SPF_VAL_LWE1 (W = k*N+1), the body is word
 * W-1.  No floating point: the words are the integers' words.  Weights live in the context like keys, in SPF_LWE_LINEAR_SLOTS
 * numbered slots; loading a slot again replaces its weights.  A load is synchronous and must not race work that uses the slot
 * (the rule of the key loads); spf_destroy frees the images.  A slot holds at most 2^27 weights (M * K): a larger matrix is
 * SPF_ERR_INVALID_ARGUMENT, with both numbers in the message.  Weights in [-8 355 711, 8 421 504] are also kept as up to three
 * balanced int8 limbs of -w for the matrix cores; any int64 is served.
 *   SPF_ERR_NO_KEY: the slot is empty.  SPF_ERR_INVALID_ARGUMENT: slot >= SPF_LWE_LINEAR_SLOTS, M or K = 0, a kind that is not
 *   an LWE kind, a null pointer, an output range that overlaps the input range.
 * spf_lwe_linear_enqueue is the form on device pointers, under the contract of the `_dev` entry points above: it only enqueues on
 * `stream`; the byte planes of the inputs live in a buffer of the context (one stream per context), which grows by the same rule.
 * "lwe_linear_planes" and "lwe_linear" of spf_last_kernel_ms time the planes pass and the product; spf_last_lwe_linear_kernel
 * names the product kernel of the last call ("pfks_gemm_kernel<U>" or "lwe_linear_valu_kernel"; the environment variable
 * SPF_LWE_LINEAR_PATH=valu|mfma, a diagnostic, forces either where both are legal).
 * The group forms: the load goes to every member, straight from the host pointer; B is dealt in contiguous shards. */
typedef enum spf_lwe_linear_limits { SPF_LWE_LINEAR_SLOTS = 64 } spf_lwe_linear_limits;
spf_status spf_load_lwe_linear_weights(spf_ctx *ctx, uint32_t slot, size_t M, size_t K, const int64_t *weights /* [M][K] */,
                                       const uint64_t *bias /* [M] or NULL */);
spf_status spf_lwe_linear_batch(spf_ctx *ctx, uint32_t slot, spf_value_kind kind, size_t B, const uint64_t *lwe_in,
                                uint64_t *lwe_out);
spf_status spf_lwe_linear_enqueue(spf_ctx *ctx, void *stream, uint32_t slot, spf_value_kind kind, size_t B,
                                  const uint64_t *d_lwe_in, uint64_t *d_lwe_out);
const char *spf_last_lwe_linear_kernel(spf_ctx *ctx);

/* ---- plaintext polynomial linear maps over GLWE ciphertexts ----------------------------------
 * `glwe_polynomial_mad` (sunscreen_tfhe/src/ops/ciphertext/glwe_ciphertext_ops.rs:164-183, over `polynomial_external_mad`,
 * math/polynomial.rs:114-197), `glwe_scalar_mad` (:189-202), `sub_glwe_ciphertexts` (:121-141), `glwe_negate_inplace` (:147-156)
 * and `glwe_rotate` (:285-305) — and the keyless NOT, addition and multiplication by X^n above — as ONE operation, for any M x K
 * matrix w of plaintext polynomials and an optional bias of M plaintext polynomials, in R = Z_2^64[X]/(X^N + 1):
 *   out[b][m][p] = sum_k w[m][k] * in[b][k][p]   for p = 0 .. glwe_size (the mask polynomials, then the body), every word mod 2^64
 *   out[b][m][glwe_size] += bias[m]
 * in [B][K][(k+1)*N], out [B][M][(k+1)*N], all SPF_VAL_GLWE1 rows.  No floating point, no key, no tolerance: the words are the
 * integers' words.  The matrix is given sparse, in CSR form over its M*K polynomials: polynomial (m, k) is the sum of
 * coefficients[t] * X^exponents[t] over t in [offsets[m*K + k], offsets[m*K + k + 1]).  Duplicate exponents inside a polynomial are
 * legal and add; a polynomial without terms is zero; any int64 coefficient is served, INT64_MIN included; exponents and
 * coefficients may be null where the matrix has no term at all (the bias alone).  Weights live in the context like keys, in
 * SPF_GLWE_POLY_SLOTS numbered slots; a load is synchronous, replaces the slot and must not race work that uses it (the rule of
 * the key loads); spf_destroy frees the images.
 *   SPF_ERR_NO_KEY: the slot is empty.  SPF_ERR_INVALID_ARGUMENT, with the offending numbers in the message: slot >=
 *   SPF_GLWE_POLY_SLOTS, M or K = 0, M > SPF_GLWE_POLY_MAX_ROWS, M * K > 2^22, offsets that do not start at 0 or that decrease,
 *   more than SPF_GLWE_POLY_MAX_TERMS terms (read from the last offset alone, before any other offset or any term is read), an
 *   exponent >= N, a null pointer, an output range that overlaps the input range.
 * spf_glwe_poly_linear_enqueue is the form on device pointers, under the contract of the `_dev` entry points above: it only
 * enqueues on `stream`, one launch whatever B, and uses no buffer of the context.  "glwe_poly_linear" of spf_last_kernel_ms times
 * it.  A slot whose every exponent is 0 (scalar weights: weighted sums, subtraction, negation, `glwe_rotate` through a constant
 * bias) is served by "glwe_poly_stream_kernel", any other by "glwe_poly_lds_kernel"; spf_last_glwe_poly_kernel names the kernel
 * of the last call (the environment variable SPF_GLWE_POLY_PATH=lds|stream, a diagnostic read at every call, forces the LDS kernel
 * on a constants-only slot; `stream` on any other slot is ignored).  spf_glwe_poly_slot_shape: M, K, the number of terms and
 * whether a bias is loaded.  The group forms: the load goes to every member, straight from the host pointers; B is dealt in
 * contiguous shards. */
typedef enum spf_glwe_poly_limits {
    SPF_GLWE_POLY_SLOTS = 64,
    SPF_GLWE_POLY_MAX_ROWS = 4096,
    SPF_GLWE_POLY_MAX_TERMS = 16777216 /* 2^24 */
} spf_glwe_poly_limits;
spf_status spf_load_glwe_poly_weights(spf_ctx *ctx, uint32_t slot, size_t M, size_t K, const uint32_t *offsets /* [M*K+1] */,
                                      const uint32_t *exponents /* [T] */, const int64_t *coefficients /* [T] */,
                                      const uint64_t *bias /* [M][N] or NULL */);
spf_status spf_glwe_poly_linear_batch(spf_ctx *ctx, uint32_t slot, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
spf_status spf_glwe_poly_linear_enqueue(spf_ctx *ctx, void *stream, uint32_t slot, size_t B, const uint64_t *d_glwe_in,
                                        uint64_t *d_glwe_out);
spf_status spf_glwe_poly_slot_shape(spf_ctx *ctx, uint32_t slot, size_t *M, size_t *K, size_t *terms, int *has_bias);
const char *spf_last_glwe_poly_kernel(spf_ctx *ctx);

/* ---- one launch over items with a parameter each ------------------------------------------------
 * The four single-operand operations that take a parameter, with the parameter PER ITEM: item i of the batch runs under
 * params[i], row i of the output is its result, every word equal to the single-parameter call's.
 *   spf_sample_extract_l1_each_*   replaces one spf_sample_extract_l1_batch / _dev call per distinct index (the 32
 *                                  `SampleExtract(i)` of a 32-bit unpack are ONE call); idx[i] < N
 *   spf_glwe_mul_xn_each_*         replaces one spf_glwe_mul_xn_batch / _dev call per distinct amount; amounts[i] taken mod 2N
 *   spf_glwe_keyswitch_each_*      replaces one spf_glwe_keyswitch_batch / _enqueue call per distinct slot; slots[i] < SPF_GLWE_KSK_SLOTS
 *   spf_glwe_automorphism_each_*   replaces one spf_glwe_automorphism_batch / _enqueue call per distinct round; rounds[i] in 1 .. log2 N
 * (the trace has no parameter).  The parameters are a HOST array of B values in every form, read during the call.
 * Launches: SampleExtract, MulXN and the automorphism round make ONE launch; the keyswitch one launch per distinct
 * (radix_log, radix_count) among the slots named — keys of different radix never share a launch.  The kernels read every operand
 * once, where it lies, through a pointer table (no gather pass); the hand-written keyswitch kernel ("glwe_ks_each_kernel", 6 x 7
 * bits at N = 2048, k = 1; elsewhere "generic_glwe_ks_each_kernel" — spf_last_glwe_keyswitch_kernel names them, "glwe_keyswitch"
 * of spf_last_kernel_ms times them) runs four items per workgroup over one key, so the items are ordered by parameter and every
 * parameter's run is padded to a whole workgroup; the results land in the caller's order all the same.
 * Before anything is queued, and touching nothing: an index >= N, a slot >= SPF_GLWE_KSK_SLOTS or a round outside 1 .. log2 N is
 * SPF_ERR_INVALID_ARGUMENT with the offending position and value in the message; an empty slot, or no automorphism key, is
 * SPF_ERR_NO_KEY; B = 0 is SPF_OK; ANY overlap of output and input — out == in too: the kernels write row i while other items are
 * still being read — is SPF_ERR_INVALID_ARGUMENT.
 * The _devptr forms (not `_dev`: unlike every `_dev` entry point they also read a host array, during the call) take device
 * pointers for the ciphertexts under the contract of the `_dev` entry points above and only enqueue on `stream`; the
 * pointer and parameter tables of a call live in a buffer of the context, so use ONE stream per context with them (a call may
 * wait until the previous call's table has left the host).  There is no _enqueue form: that contract allows no buffer of the
 * context.  (SPF_GLWE_KSK_SLOTS, the key slots and spf_last_glwe_keyswitch_kernel: the next section.)  The group forms deal the parameter array in the same contiguous shards as the items. */
spf_status spf_sample_extract_l1_each_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in, const uint64_t *idx, uint64_t *lwe1_out);
spf_status spf_sample_extract_l1_each_devptr(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_glwe_in, const uint64_t *idx,
                                          uint64_t *d_lwe1_out);
spf_status spf_glwe_mul_xn_each_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in, const uint64_t *amounts, uint64_t *glwe_out);
spf_status spf_glwe_mul_xn_each_devptr(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_glwe_in, const uint64_t *amounts,
                                    uint64_t *d_glwe_out);
spf_status spf_glwe_keyswitch_each_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in, const uint64_t *slots, uint64_t *glwe_out);
spf_status spf_glwe_keyswitch_each_devptr(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_glwe_in, const uint64_t *slots,
                                       uint64_t *d_glwe_out);
spf_status spf_glwe_automorphism_each_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in, const uint64_t *rounds, uint64_t *glwe_out);
spf_status spf_glwe_automorphism_each_devptr(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_glwe_in, const uint64_t *rounds,
                                          uint64_t *d_glwe_out);

/* ---- GLWE keyswitch, one automorphism round, homomorphic trace ---------------------------------
 * The three functions the circuit bootstrap's trace is built from, on B GLWEs of (k+1)*N words each (SPF_VAL_GLWE1 rows), B
 * GLWEs out:
 *   spf_glwe_keyswitch_*     `keyswitch_glwe_to_glwe` (sunscreen_tfhe/src/ops/fft_ops.rs:457-495; integer twin
 *                            ops/keyswitch/glwe_keyswitch.rs:26-55) under the key in `slot`:
 *                            out = (0, .., 0, b) - sum_i <decomp(a_i), KSK_i>
 *   spf_glwe_automorphism_*  one round of the trace's loop (ops/automorphisms/mod.rs:72-83), `round` in 1 .. log2 N:
 *                            out = keyswitch(in(X^t), ak[round-1]), t = N / 2^(round-1) + 1 (`polynomial_pow_k`,
 *                            ops/polynomial/mod.rs:62-84), under the context's automorphism key and tr_radix
 *   spf_glwe_trace_*         `trace` (ops/automorphisms/mod.rs:53-85): x <- x + automorphism_round(x) for rounds 1 .. log2 N in turn
 * Every word equals the reference's: the kernels run its arithmetic in its order (spf_mod_switch_trace_and_rotate_* runs the same
 * trace behind the circuit bootstrap's own prologue).
 * Keys: SPF_GLWE_KSK_SLOTS numbered slots in the context.  spf_load_glwe_keyswitch_key_std takes a `GlweKeyswitchKey<u64>` in
 * integer form, [row<k][level<radix_count][poly<k+1][N] words — n_words must be exactly k * radix_count * (k+1) * N — and transforms
 * it on the device as spf_load_automorphism_key_std does; the radix comes with the key.  The load is synchronous, replaces what the
 * slot held and must not race work that uses the slot (the rule of the key loads); spf_destroy frees the slots.
 * SPF_ERR_INVALID_ARGUMENT, with the offending numbers in the message and nothing touched: slot >= SPF_GLWE_KSK_SLOTS, radix_log or
 * radix_count = 0, radix_log * radix_count > 64 — and = 64, which the reference accepts and the kernels do not (they round to the
 * top radix_log * radix_count bits by the bit below them) —, another n_words.  spf_glwe_keyswitch_slot_shape reads the radix back;
 * an empty slot is SPF_ERR_NO_KEY.
 * Statuses of the operations: B = 0 is SPF_OK; an empty slot, or no automorphism key, is SPF_ERR_NO_KEY; a round outside
 * 1 .. log2 N or a slot >= SPF_GLWE_KSK_SLOTS is SPF_ERR_INVALID_ARGUMENT before anything is queued.
 * Aliasing: glwe_out == glwe_in EXACTLY (the same address: the operation runs in place) is allowed; any other overlap of the two
 * ranges is the caller's error and is refused with SPF_ERR_INVALID_ARGUMENT.
 * The _enqueue forms take device pointers under the contract of the `_dev` entry points above: they only enqueue on `stream`, ONE
 * launch whatever B (B <= 2^31 - 1), and use no buffer of the context.  "glwe_keyswitch" of spf_last_kernel_ms times all three.
 * N = 2048, k = 1 with a radix of 6 levels x 7 bits (DEFAULT_128's automorphism key) runs the hand-written "glwe_ks_kernel",
 * every other shape — a generic context, or another radix on a tuned one — "generic_glwe_ks_kernel";
 * spf_last_glwe_keyswitch_kernel names the kernel of the last call (the nodes of a gate graph, spf_graph_add_glwe_keyswitch below,
 * add "glwe_ks_rows_kernel" and "generic_glwe_ks_rows_kernel").  The group forms: the key goes to every member, B is dealt in
 * contiguous shards. */
typedef enum spf_glwe_ksk_limits { SPF_GLWE_KSK_SLOTS = 16 } spf_glwe_ksk_limits;
spf_status spf_load_glwe_keyswitch_key_std(spf_ctx *ctx, uint32_t slot, const uint64_t *key, size_t n_words, uint32_t radix_log,
                                           uint32_t radix_count);
spf_status spf_glwe_keyswitch_slot_shape(spf_ctx *ctx, uint32_t slot, uint32_t *radix_log, uint32_t *radix_count);
spf_status spf_glwe_keyswitch_batch(spf_ctx *ctx, uint32_t slot, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
spf_status spf_glwe_keyswitch_enqueue(spf_ctx *ctx, void *stream, uint32_t slot, size_t B, const uint64_t *d_glwe_in,
                                      uint64_t *d_glwe_out);
spf_status spf_glwe_automorphism_batch(spf_ctx *ctx, uint32_t round, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
spf_status spf_glwe_automorphism_enqueue(spf_ctx *ctx, void *stream, uint32_t round, size_t B, const uint64_t *d_glwe_in,
                                         uint64_t *d_glwe_out);
spf_status spf_glwe_trace_batch(spf_ctx *ctx, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
spf_status spf_glwe_trace_enqueue(spf_ctx *ctx, void *stream, size_t B, const uint64_t *d_glwe_in, uint64_t *d_glwe_out);
const char *spf_last_glwe_keyswitch_kernel(spf_ctx *ctx);

/* ---- call coalescing: many threads, one ciphertext each -> one batch per launch ----------
 * The reference calls `Evaluation` from many rayon workers with a single ciphertext per call
 * (circuit_processor/mod.rs:192-253).  A pool keeps that calling convention — submit, then wait like the synchronous call it
 * replaces — and runs what has gathered of one kind as ONE batch.
 *   Buffers: the INPUT is copied into the pool's pinned staging during submit (it may be released when submit returns); the
 *     OUTPUT buffer must stay valid until spf_pool_wait returns for its ticket — or, for a ticket nobody waits for, until the
 *     pool is destroyed: an output left uncollected for 200 ms is written to its buffer by a pool thread so that the staging
 *     set can be reused (a later wait still returns the status, and never returns while that copy is in progress).
 *   Batching: a calling thread is dealt to one of up to four caller groups on its first submit and stays there; a group's
 *     batch closes when it is full (max_batch, and the staging a batch may pin), when every caller of the group's previous
 *     batch is back, or when nobody has joined it for max_wait_us (stretched to an eighth of the last batch's GPU time, at most
 *     twenty such quiet times after its first member) — but not on the timer while the group's previous batch is still out.
 *     The groups' batches run on the GPU side by side, each on its own stream (profiles/r05_pool.md).
 *   Asynchronous use: a thread may hold many tickets; sixteen staging sets exist (spf_pool_counters.staging_sets), so a caller
 *     that keeps more than sixteen host-pointer batches uncollected waits in submit until a set is collected (or 200 ms old).
 *     Batches by handle give their set back when they complete.
 *   spf_pool_wait returns the status of the batch the operation ran in (first-error-wins per batch, as
 *     circuit_processor/mod.rs:214-223 does per graph).
 *   The library asks the HIP runtime for more hardware queues when it is loaded (GPU_MAX_HW_QUEUES=24 unless set): streams that
 *   share a hardware queue run their kernels one after the other. */
typedef struct spf_pool spf_pool;
/* (the pool retains `ctx` until spf_pool_destroy: see Lifetimes at spf_create) */
spf_status spf_pool_create(spf_ctx *ctx, size_t max_batch, uint32_t max_wait_us, spf_pool **out);
void spf_pool_destroy(spf_pool *pool); /* drains pending work first */
/* `Evaluation::keyswitch_lwe_l1_lwe_l0` for one ciphertext */
spf_status spf_pool_submit_keyswitch(spf_pool *pool, const uint64_t *lwe1_in, uint64_t *lwe0_out, uint64_t *ticket);
/* `Evaluation::circuit_bootstrap` for one ciphertext */
spf_status spf_pool_submit_circuit_bootstrap(spf_pool *pool, const uint64_t *lwe0_in, double *ggsw_fft_out,
                                             uint64_t *ticket);
/* FheOp::KeyswitchL1toL0 -> FheOp::CircuitBootstrap for one ciphertext (L1 LWE in, L1 GGSW out) */
spf_status spf_pool_submit_keyswitch_circuit_bootstrap(spf_pool *pool, const uint64_t *lwe1_in,
                                                       double *ggsw_fft_out, uint64_t *ticket);
/* `KeylessEvaluation::cmux` for one gate */
spf_status spf_pool_submit_cmux(spf_pool *pool, const double *sel_ggsw_fft, const uint64_t *a, const uint64_t *b,
                                uint64_t *out, uint64_t *ticket);
/* The other operations `CircuitProcessor::exec_op` issues per task (circuit_processor/mod.rs:341-540), one ciphertext per call:
 *   FheOp::SampleExtract(idx) -> `KeylessEvaluation::sample_extract_l1` (crypto/evaluation.rs:126-133); idx >= N is
 *                                SPF_ERR_INVALID_ARGUMENT.  Calls with different indices run in different batches
 *                                unless the pool mixes parameters (spf_pool_set_mixed_parameters below).
 *   FheOp::Not / GlweAdd / MulXN(n) -> `not` / `xor` / `mul_xn` (crypto/evaluation.rs:47-66); n is taken mod 2N (calls with
 *                                different amounts: as for the indices)
 *   FheOp::MultiplyGgswGlwe -> `multiply_glwe_ggsw` (:104-123)         FheOp::GlevCMux -> `glev_cmux` (:86-101), GLEVs of l_cbs GLWEs
 *   FheOp::SchemeSwitch -> `Evaluation::scheme_switch` (:231-240) */
spf_status spf_pool_submit_sample_extract(spf_pool *pool, const uint64_t *glwe_in, size_t idx, uint64_t *lwe1_out, uint64_t *ticket);
spf_status spf_pool_submit_not(spf_pool *pool, const uint64_t *glwe_in, uint64_t *glwe_out, uint64_t *ticket);
spf_status spf_pool_submit_glwe_add(spf_pool *pool, const uint64_t *a, const uint64_t *b, uint64_t *glwe_out, uint64_t *ticket);
spf_status spf_pool_submit_mul_xn(spf_pool *pool, const uint64_t *glwe_in, size_t n, uint64_t *glwe_out, uint64_t *ticket);
spf_status spf_pool_submit_multiply_ggsw_glwe(spf_pool *pool, const double *ggsw_fft, const uint64_t *glwe, uint64_t *glwe_out,
                                              uint64_t *ticket);
spf_status spf_pool_submit_glev_cmux(spf_pool *pool, const double *sel_ggsw_fft, const uint64_t *a, const uint64_t *b,
                                     uint64_t *glev_out, uint64_t *ticket);
spf_status spf_pool_submit_scheme_switch(spf_pool *pool, const uint64_t *glev_in, double *ggsw_fft_out, uint64_t *ticket);
/* `keyswitch_glwe_to_glwe` under the key of `slot`, one round of the trace's loop and `trace` (spf_glwe_keyswitch_batch /
 * spf_glwe_automorphism_batch / spf_glwe_trace_batch above) for one GLWE; word-equal to those.  Calls with different slots or
 * rounds run in different batches unless the pool mixes parameters (spf_pool_set_mixed_parameters below).  Checked at the submit: slot >= SPF_GLWE_KSK_SLOTS, round 0 or round > log2 N are
 * SPF_ERR_INVALID_ARGUMENT; an empty slot, or no automorphism key, is SPF_ERR_NO_KEY; a refused call takes no ticket.
 * The batch reads the slot again when it is launched.  Reloading a slot (spf_load_glwe_keyswitch_key_std, or the automorphism
 * key) while submissions that use it are outstanding is the caller's error, as for every key loader: WAIT for every ticket and
 * value submitted on the slot first, then load, then submit again.  The same holds by handle (below). */
spf_status spf_pool_submit_glwe_keyswitch(spf_pool *pool, uint32_t slot, const uint64_t *glwe_in, uint64_t *glwe_out, uint64_t *ticket);
spf_status spf_pool_submit_glwe_automorphism(spf_pool *pool, uint32_t round, const uint64_t *glwe_in, uint64_t *glwe_out,
                                             uint64_t *ticket);
spf_status spf_pool_submit_glwe_trace(spf_pool *pool, const uint64_t *glwe_in, uint64_t *glwe_out, uint64_t *ticket);
/* Blocks until the operation has run; each ticket can be collected exactly once (an unknown or already
 * collected ticket is SPF_ERR_INVALID_ARGUMENT, never a hang). */
spf_status spf_pool_wait(spf_pool *pool, uint64_t ticket);
/* Flow control (the reference bounds its in-flight operations with a token channel,
 * circuit_processor/mod.rs:139): a submit blocks while `max_inflight` tickets are submitted and not yet
 * collected.  Default 4 x max_batch. */
spf_status spf_pool_set_max_inflight(spf_pool *pool, size_t max_inflight);
/* Mixed parameters, opt-in (`on` != 0; the default is off and changes nothing): SampleExtract, MulXN, GLWE keyswitch and
 * automorphism calls with DIFFERENT indices, amounts, slots or rounds join the same batch — by host pointer and by handle, on
 * valid and on pending operands — and the batch runs as ONE launch of the per-item kernels (spf_*_each_* above) over its members'
 * parameters: the 32 `SampleExtract(i)` of a 32-bit unpack are one launch, not 32.  A keyswitch batch holds slots of ONE
 * (radix_log, radix_count), as read at the submit: keys of different radix never share a launch.  Every other operation batches
 * as before (a blind rotation's steps sit at different depths and never meet; a bivariate bootstrap's plaintext_bits are a
 * constant of a workload).  Results are word-equal to the pool without it.  Legal only before the pool's first submit:
 * afterwards SPF_ERR_INVALID_ARGUMENT.  A group pool applies it to every member.  The rule for reloading a key slot is unchanged. */
spf_status spf_pool_set_mixed_parameters(spf_pool *pool, int on);
/* operations completed and batches launched so far (ops / launches = achieved batch size) */
spf_status spf_pool_stats(spf_pool *pool, uint64_t *ops, uint64_t *launches);

/* counters of a pool (sums over the members of a group pool) */
typedef struct spf_pool_counters {
    uint64_t ops, launches;                  /* as spf_pool_stats: operations completed, batches launched (both forms) */
    uint64_t handle_ops, handle_launches;    /* ... of which by handle */
    uint64_t reclaimed;                      /* outputs a pool thread delivered on behalf of a caller that never collected them */
    uint64_t bootstrap_launches_by_shape[3]; /* circuit-bootstrap batches by blind-rotation shape: eight waves per ciphertext
                                              * (blind_rotate8), two ciphertexts per workgroup (2p2), four (2p) */
    uint64_t staging_sets;                   /* staging sets per pool (a caller may leave that many batches uncollected) */
    uint64_t value_mallocs;                  /* hipMalloc calls of the value arena so far (steady state: no growth) */
    uint64_t stream_concurrency;             /* how many of the pool's streams ran side by side in the probe spf_pool_create makes
                                              * (a 200 us spin kernel on every set's stream at once; minimum over the members;
                                              * the best of three probes).  At 5 or below the resident batches take turns: GPU_MAX_HW_QUEUES took effect too late
                                              * (a host that touched HIP before loading the library) — spf_pool_create then
                                              * still returns SPF_OK and leaves a WARNING in spf_last_error(ctx) */
} spf_pool_counters;
spf_status spf_pool_counters_get(spf_pool *pool, spf_pool_counters *out);

/* ---- device-resident values: the per-operation boundary without PCIe (SURVEY.md §8 b / f3) ---------------------------- *
 *
 * `CircuitProcessor::exec_op` calls `Evaluation` once per `FheOp` (circuit_processor/mod.rs:255-540) with ciphertexts that
 * live in host memory (crypto/encryption.rs:143-165); the GGSW a `CircuitBootstrap` produces is consumed by the ~45 CMux
 * gates behind it (fhe_circuit.rs:473-494).  Through the host-pointer submits above every operand and result crosses PCIe on
 * every call (a CMux: 256 KiB + 2 x 32 KiB in, 32 KiB out).  A *value* is a reference-counted ciphertext in the HBM of one
 * context; the `_v` submits take values and return a value, and nothing crosses PCIe until spf_value_download.  A Rust shim
 * keeps an `Option<SpfValue>` beside (or instead of) the host copy inside `L1GgswCiphertext` & co..
 *
 *   Lifetime: every value returned through an `out` parameter carries ONE reference owned by the caller; spf_value_release
 *     drops it (spf_value_retain adds one).  The pool keeps operands alive while an operation that reads them is queued or
 *     running, so a caller may release an operand right after the submit that used it.  Values may outlive their pool (their
 *     memory is freed on release); they must not be USED with another pool.
 *   Validity: a result value exists as soon as the submit returns, but becomes valid only when its operation has run:
 *     spf_pool_wait has returned SPF_OK for its ticket — exactly when the reference's task output becomes visible to its
 *     dependents (circuit_processor/mod.rs:214-246) — or spf_value_wait has returned SPF_OK for the value.  Reading it earlier
 *     (spf_value_download, spf_value_device_ptr, spf_value_copy_to_member), or after a failed batch, is
 *     SPF_ERR_INVALID_ARGUMENT, never a read of unfinished data.  It must be released in every case.
 *   Deferred operands: a result that is still pending MAY be passed as an operand of a later `_v` submit to the same pool.  The
 *     pool orders the two on the device (stream order, events, or — behind a bootstrap batch — launching the dependent batch
 *     when the producing one has finished) and batches what has been pushed by level: operations on pending operands join the
 *     open batch of their (depth, kind, parameter), depth = 1 + the deepest batch an operand comes from (the bootstrap kinds:
 *     one batch per number of bootstraps they are behind, whatever the depth), and the table is launched in dependency order
 *     when a result in it is waited for or when nothing has joined it for max_wait_us.  A caller can thus push a whole circuit —
 *     every `FheOp` one `_v` submit, from one thread, without a single wait — and wait for the outputs only: the level batching
 *     of spf_graph_run, built while the operations arrive.  An operation whose operand's producer failed fails with that status.
 *     `ticket` may be NULL in the `_v` submits: nobody will spf_pool_wait for that operation (no ticket to collect, no
 *     back-pressure from it); spf_value_wait on the result, or on anything computed from it, takes its place.
 *   Placement: a value lives on ONE member of a group pool (member 0 of a plain pool).  `member` < 0 in spf_value_upload /
 *     spf_value_trivial = the calling thread's home member (as the host-pointer submits deal their callers); an operation
 *     runs on the member its operands live on, its result stays there; operands on different members are
 *     SPF_ERR_INVALID_ARGUMENT — spf_value_copy_to_member makes a copy on another member (peer copy over xGMI).
 *   Memory: the results of one batch share one block of the pool's arena (the kernels write consecutive rows); the block is
 *     reused when its last value is released, so a value pins the block of its batch mates.  Blocks are cached (never
 *     hipFree'd on the steady-state path: hipFree waits for the whole device); spf_pool_trim gives the cache back to the
 *     driver, spf_pool_value_stats reports live values, live bytes (blocks handed out) and cached bytes.
 *     Environment: SPF_VALUE_CACHE_MB bounds the cache (default 32768). */
typedef struct spf_value spf_value;
/* host -> HBM: `host` holds one ciphertext of `kind` in the layout of the conventions above (spf_ciphertext_words(kind) u64
 * words; SPF_VAL_GGSW1: (k+1)*l_cbs*(k+1)*N/2 complex) */
spf_status spf_value_upload(spf_pool *pool, int member, spf_value_kind kind, const void *host, spf_value **out);
/* n ciphertexts of one kind (the bits of an encrypted integer: `host` holds them consecutively) into ONE block with one copy;
 * out receives n values.  Operations that take them in order find them consecutive in HBM (no packing pass). */
spf_status spf_value_upload_batch(spf_pool *pool, int member, spf_value_kind kind, size_t n, const void *host, spf_value **out);
/* n valid values of one kind on one member -> `host`, consecutively (blocking): one copy when they lie consecutively in one block
 * (the results of one batch in slot order, or of spf_value_upload_batch), one copy each otherwise */
spf_status spf_value_download_batch(size_t n, const spf_value *const *values, void *host);
/* FheOp::{Zero,One}{Lwe0,Glwe1,Glev1,Ggsw1} (fhe_circuit.rs:96-116; also LWE1) as values: the trivial encryption of `bit`; the
 * GGSW constants are `Evaluation::l1ggsw_zero / l1ggsw_one` (crypto/evaluation.rs:254-262) and need all four keys */
spf_status spf_value_trivial(spf_pool *pool, int member, spf_value_kind kind, uint64_t bit, spf_value **out);
/* HBM -> host (blocking); `host` has room for the kind's words */
spf_status spf_value_download(const spf_value *value, void *host);
/* blocks until the operation that produces `value` has run (returns at once for a valid value): SPF_OK, or the failure;
 * any thread, any number of times, whether or not the operation has a ticket.  Launches what the value needs: the deferred table,
 * or the open batch the operation sits in (spf_pool_wait leaves such a batch open for other callers to join). */
spf_status spf_value_wait(const spf_value *value);
/* launches what has been pushed so far (the deferred table, see Deferred operands) without waiting for anything: a pusher that
 * knows a long operation is complete — the conversions at the head of a circuit — lets it start while it pushes the rest */
spf_status spf_pool_flush(spf_pool *pool);
spf_status spf_value_retain(spf_value *value);
void spf_value_release(spf_value *value);
/* any of the out pointers may be NULL */
spf_status spf_value_info(const spf_value *value, spf_value_kind *kind, size_t *bytes, int *member, int *valid);
/* the device address of a valid value, for a caller that chains the `_dev` entry points on the member's context
 * (spf_group_ctx); stays valid while the caller holds its reference */
spf_status spf_value_device_ptr(const spf_value *value, void **dev_ptr);
/* a copy of a valid value on `member` of the group pool (device-to-device on the same GPU, peer copy otherwise; blocking) */
spf_status spf_value_copy_to_member(spf_pool *pool, const spf_value *value, int member, spf_value **out);
spf_status spf_pool_value_stats(spf_pool *pool, size_t *live_values, size_t *live_bytes, size_t *cached_bytes);
spf_status spf_pool_trim(spf_pool *pool);

/* The pool's submits by handle: same operations, same batching, same spf_pool_wait as the host-pointer forms above; operands
 * are values of this pool — valid, or still pending (see Deferred operands) —, *out receives the result value (see Validity),
 * `ticket` may be NULL.  Batches by handle never mix with host-pointer callers.  No staging, no copies: the CMUX family reads its operands where they are, the other kinds pack theirs on the device
 * (gather_rows_kernel) unless they already lie consecutively. */
spf_status spf_pool_submit_keyswitch_v(spf_pool *pool, const spf_value *lwe1, spf_value **lwe0_out, uint64_t *ticket);
spf_status spf_pool_submit_circuit_bootstrap_v(spf_pool *pool, const spf_value *lwe0, spf_value **ggsw_out, uint64_t *ticket);
spf_status spf_pool_submit_keyswitch_circuit_bootstrap_v(spf_pool *pool, const spf_value *lwe1, spf_value **ggsw_out,
                                                         uint64_t *ticket);
spf_status spf_pool_submit_cmux_v(spf_pool *pool, const spf_value *sel_ggsw, const spf_value *a, const spf_value *b,
                                  spf_value **out, uint64_t *ticket);
spf_status spf_pool_submit_sample_extract_v(spf_pool *pool, const spf_value *glwe, size_t idx, spf_value **lwe1_out,
                                            uint64_t *ticket);
spf_status spf_pool_submit_not_v(spf_pool *pool, const spf_value *glwe, spf_value **out, uint64_t *ticket);
spf_status spf_pool_submit_glwe_add_v(spf_pool *pool, const spf_value *a, const spf_value *b, spf_value **out, uint64_t *ticket);
spf_status spf_pool_submit_mul_xn_v(spf_pool *pool, const spf_value *glwe, size_t n, spf_value **out, uint64_t *ticket);
spf_status spf_pool_submit_multiply_ggsw_glwe_v(spf_pool *pool, const spf_value *ggsw, const spf_value *glwe, spf_value **out,
                                                uint64_t *ticket);
spf_status spf_pool_submit_glev_cmux_v(spf_pool *pool, const spf_value *sel_ggsw, const spf_value *a, const spf_value *b,
                                       spf_value **glev_out, uint64_t *ticket);
spf_status spf_pool_submit_scheme_switch_v(spf_pool *pool, const spf_value *glev, spf_value **ggsw_out, uint64_t *ticket);
/* GLWE keyswitch, one automorphism round and trace by handle (the statuses and the reload rule of spf_pool_submit_glwe_keyswitch
 * above; a refused call creates no value: *out is not written).  The operand may be valid or still pending.  A batch whose
 * operands lie consecutively in device memory runs the in-place kernel on them, any other ONE launch of the rows kernel over a
 * table of their addresses — nothing is copied (spf_last_glwe_keyswitch_kernel tells which; the environment variable
 * SPF_GLWE_KS_ROWS_GATHER=1, a diagnostic read by spf_pool_create, packs the operands first as the other kinds do).  The results of a
 * batch are fresh memory: they overlap no operand, and one value may be the operand of several operations of a batch. */
spf_status spf_pool_submit_glwe_keyswitch_v(spf_pool *pool, uint32_t slot, const spf_value *glwe, spf_value **out, uint64_t *ticket);
spf_status spf_pool_submit_glwe_automorphism_v(spf_pool *pool, uint32_t round, const spf_value *glwe, spf_value **out,
                                               uint64_t *ticket);
spf_status spf_pool_submit_glwe_trace_v(spf_pool *pool, const spf_value *glwe, spf_value **out, uint64_t *ticket);
/* `blind_rotation` (blind_rotation.rs:202-223) by handle: *out = glwe * X^-(s << log_stride), s given as the n_bits glwe-level
 * GGSW values of its bits (bit 0 first; valid or still pending, e.g. results of spf_pool_submit_keyswitch_circuit_bootstrap_v;
 * repeats allowed).  Word-equal to spf_blind_rotation_batch.  n_bits >= 1 and n_bits + log_stride <= log2(polynomial_degree);
 * operands on different members of a group are SPF_ERR_INVALID_ARGUMENT, a tuned context whose cbs radix is not 4 x 4 bits
 * SPF_ERR_UNSUPPORTED; everything is checked before anything is queued.  One step per bit is queued, each on the pending result
 * of the one before: step i of every caller that pushed the same (i, log_stride) is ONE launch over a pointer table.  The
 * intermediate values are the library's; `ticket` (may be NULL) is the last step's. */
spf_status spf_pool_submit_blind_rotation_v(spf_pool *pool, const spf_value *glwe, const spf_value *const *shift_ggsw /* n_bits */,
                                            size_t n_bits, size_t log_stride, spf_value **out, uint64_t *ticket);
/* `exec_op`'s whole match in one entry (circuit_processor/mod.rs:255-540): the operation as a spf_graph_op, operands in the order
 * spf_graph_add_op takes them (CMUX: selector, low, high), `param` = SampleExtract index / MulXN amount.  SPF_OP_PBS_UNIVARIATE
 * [lwe0, lut glwe1] and SPF_OP_PBS_BIVARIATE [left lwe0, right lwe0, lut glwe1] (`param` = plaintext_bits < 64) go the same
 * way: `programmable_bootstrap_univariate` / `_bivariate` (programmable_bootstrapping.rs:291, 575-621) by handle, batched and paced
 * like the circuit bootstraps, word-equal to spf_pbs_univariate_batch / spf_pbs_bivariate_batch of the same rows.
 * SPF_OP_GLWE_KEYSWITCH (`param` = slot), SPF_OP_GLWE_AUTOMORPHISM (`param` = round) and SPF_OP_GLWE_TRACE [glwe1] are the three
 * submits above. */
spf_status spf_pool_submit_op_v(spf_pool *pool, spf_graph_op op, const spf_value *const *inputs, size_t n_inputs, uint64_t param,
                                spf_value **out, uint64_t *ticket);

/* ---- gate graphs: level-batched, device-resident execution ------------- *
 *
 * The counterpart of `FheCircuit` + `CircuitProcessor::run_graph_blocking`
 * (parasol_runtime/src/fhe_circuit.rs:34-126, circuit_processor/mod.rs:573-623): build a DAG of
 * `FheOp`-like nodes, then run it.  Execution is by topological level: all nodes of one level
 * and one kind are ONE batched launch, intermediates never leave HBM, the whole graph is
 * enqueued on one stream.  Node ids are dense, in creation order; operands must already exist
 * (so the node order is a topological order).  Operand order per operation:
 *   SAMPLE_EXTRACT(param = index) [glwe1] -> lwe1      KEYSWITCH_L1_TO_L0 [lwe1] -> lwe0
 *   CIRCUIT_BOOTSTRAP [lwe0] -> ggsw1                  SCHEME_SWITCH [glev1] -> ggsw1
 *   NOT [glwe1]   GLWE_ADD [glwe1, glwe1]   MUL_XN(param = n) [glwe1]           -> glwe1
 *   CMUX [sel ggsw1, low glwe1 (taken when sel = 0), high glwe1] -> glwe1   (FheEdge::Sel/Low/High)
 *   GLEV_CMUX [sel ggsw1, low glev1, high glev1] -> glev1
 *   MULTIPLY_GGSW_GLWE [ggsw1, glwe1] -> glwe1
 *   PBS_UNIVARIATE [lwe0, lut glwe1] -> lwe1           PBS_BIVARIATE(param = plaintext_bits < 64) [left lwe0, right lwe0, lut glwe1] -> lwe1
 * The two bootstraps by a caller's table stand for `programmable_bootstrap_univariate` / `programmable_bootstrap_bivariate`
 * (ops/bootstrapping/programmable_bootstrapping.rs:291, 575-621), which the reference's `FheOp` does not have: a node is word-equal to
 * spf_pbs_univariate_batch / spf_pbs_bivariate_batch of the same rows with lut_stride = one GLWE, whatever batch it lands in.
 * The table is a glwe1 node like any other (an input, a trivial encryption, something the graph computed); the nodes of a level
 * that name ONE table node read it in place.  PBS_BIVARIATE with plaintext_bits >= 64 is SPF_ERR_INVALID_ARGUMENT.
 *   GLWE_KEYSWITCH(param = slot) [glwe1]   GLWE_AUTOMORPHISM(param = round) [glwe1]   GLWE_TRACE [glwe1]   -> glwe1
 * are the nodes of spf_graph_add_glwe_keyswitch / _automorphism / _trace below, built by the same code: same checks, same groups,
 * same words.  These three values name an operation here over ONE operand only: with any other count the call is refused as
 * "unknown operation" (with the value and the count), not as a wrong number of operands.
 * Wrong arity or operand type is reported by spf_graph_add_op, before anything runs (the
 * reference validates per task, task.rs:26-31).  Input and output host buffers are read /
 * written by every spf_graph_run and must stay valid until it returns; a graph can be run
 * repeatedly with new input contents.  A graph is not thread-safe; distinct graphs on one
 * context may run from different threads (their launches serialise on the context's stream). */
typedef struct spf_graph spf_graph;
/* (the graph retains `ctx` until spf_graph_destroy: see Lifetimes at spf_create) */
spf_status spf_graph_create(spf_ctx *ctx, spf_graph **out);
void spf_graph_destroy(spf_graph *graph);
/* FheOp::Input{Lwe0,Lwe1,Glwe1,Ggsw1,Glev1} */
spf_status spf_graph_add_input(spf_graph *graph, spf_value_kind kind, const void *host, uint32_t *node);
/* FheOp::{Zero,One}{Lwe0,Glwe1,Glev1,Ggsw1} (fhe_circuit.rs:96-116; also LWE1): trivial encryption of a bit;
 * the GGSW constants are the context's circuit bootstraps of the trivial L0 LWE (Evaluation::l1ggsw_zero /
 * l1ggsw_one, crypto/evaluation.rs:161-197, 254-262) and need the bootstrap, automorphism and scheme-switch keys */
spf_status spf_graph_add_trivial(spf_graph *graph, spf_value_kind kind, uint64_t bit, uint32_t *node);
spf_status spf_graph_add_op(spf_graph *graph, spf_graph_op op, const uint32_t *inputs, size_t n_inputs,
                            uint64_t param, uint32_t *node);
/* Packed integers in and out of a graph (an n-bit integer in one L1 GLWE, bit i at X^i: see spf_glwe_pack_batch).  Node
 * constructors, not operations — as in the reference, where `PackedGenericInt::graph_input(ctx).unpack(ctx)` and
 * `.pack(ctx, enc).collect_output(ctx, enc)` are nodes of the fluent layer and no `FheOp`s (fluent/generic_int.rs:261,
 * fluent/packed_dynamic_generic_int_graph_node.rs:24-60, fluent/dynamic_generic_int_graph_nodes.rs:139-200).
 *   add_unpack: `glwe_node` is any glwe1 node (input or computed), 0 < n_bits <= polynomial_degree; creates n_bits lwe1 nodes,
 *     nodes_out[i] word-equal to SAMPLE_EXTRACT(param = i) of glwe_node, one level above it.  All unpacks of a level with the
 *     same n_bits are ONE launch (SAMPLE_EXTRACT nodes batch by index: n_bits launches).
 *   add_pack: nodes[0 .. n_bits) are glwe1 nodes of any origin and level, repeats allowed; creates one glwe1 node
 *     = sum over i of X^i * nodes[i] mod 2^64, word-equal to spf_glwe_pack_batch of those rows (and so to the reference's
 *     MulXN(i) + GlweAdd tree), one level above its highest operand.  All packs of a level with the same n_bits are ONE launch
 *     that reads the rows where they lie.
 * The new nodes are ordinary: operands of any operation, outputs, counted by spf_graph_stats.  A wrong argument
 * (n_bits out of range, a node that does not exist or is no glwe1, a null pointer) is SPF_ERR_INVALID_ARGUMENT from the call,
 * and the graph stays usable. */
spf_status spf_graph_add_unpack(spf_graph *graph, uint32_t glwe_node, size_t n_bits, uint32_t *nodes_out /* n_bits */);
spf_status spf_graph_add_pack(spf_graph *graph, const uint32_t *nodes, size_t n_bits, uint32_t *node_out);
/* `blind_rotation` (ops/bootstrapping/blind_rotation.rs:202-223) as a node constructor — no FheOp there, no spf_graph_op here:
 * creates n_bits chained glwe1 nodes acc_{i+1} = cmux(shift_nodes[i], acc_i, X^-(2^(i + log_stride)) * acc_i) with
 * acc_0 = glwe_node, so that *node_out (the last one) = glwe_node * X^-(s << log_stride), s = the integer whose bits the ggsw1
 * nodes shift_nodes[0 .. n_bits) encrypt (bit 0 first; inputs, trivial GGSWs or CIRCUIT_BOOTSTRAP results at any level, repeats
 * allowed).  Word-equal to spf_blind_rotation_batch and to MUL_XN(2N - 2^(i + log_stride)) + CMUX nodes.  Each node is one
 * level above the higher of its two operands and writes its own row; all such nodes of one level with one rotation amount are
 * ONE launch whose high operand is a rotated read of the low one.  The new nodes are ordinary glwe1 nodes.  n_bits >= 1 and
 * n_bits + log_stride <= log2(polynomial_degree); a wrong argument is SPF_ERR_INVALID_ARGUMENT from the call (a tuned context
 * whose cbs radix is not 4 x 4 bits: SPF_ERR_UNSUPPORTED), nothing is recorded and the graph stays usable. */
spf_status spf_graph_add_blind_rotation(spf_graph *graph, uint32_t glwe_node, const uint32_t *shift_nodes /* n_bits ggsw1 nodes, bit 0 first */,
                                        size_t n_bits, size_t log_stride, uint32_t *node_out);
/* `public_functional_keyswitch` (ops/keyswitch/public_functional_keyswitch.rs:74-148) with the map "message j to coefficient j"
 * as a node constructor — no FheOp there, no spf_graph_op here: lwe_nodes[0 .. lwe_count) are all lwe0 or all lwe1 nodes of any
 * origin and level (sample extracts, bootstrap results, keyswitch results, inputs; repeats allowed), 0 < lwe_count <=
 * polynomial_degree; creates ONE glwe1 node, one level above its highest operand, word-equal to
 * spf_public_functional_keyswitch_batch of those rows in that order.  All such nodes of one level with one (lwe_count, operand
 * kind) are one main launch that reads the rows where they lie.  The new node is an ordinary glwe1 node.  A wrong argument
 * (lwe_count out of range, lwe0 and lwe1 mixed, a node that does not exist or is no LWE, a null pointer) is
 * SPF_ERR_INVALID_ARGUMENT from the call, nothing is recorded and the graph stays usable.  spf_graph_run reports SPF_ERR_NO_KEY
 * while no public functional keyswitch key is loaded, and SPF_ERR_INVALID_ARGUMENT when the key's from_dimension is not the
 * dimension of the operands (lwe_dimension for lwe0, glwe_size * polynomial_degree for lwe1). */
spf_status spf_graph_add_public_functional_keyswitch(spf_graph *graph, const uint32_t *lwe_nodes, size_t lwe_count, uint32_t *node_out);
/* The plaintext linear map of weight slot `slot` (spf_load_lwe_linear_weights above) as a node constructor — no FheOp there, no
 * spf_graph_op here: what stands between two SPF_OP_PBS_* nodes (a layer, then its activation table).  lwe_nodes[0 .. K) are all
 * lwe0 or all lwe1 nodes of any origin and level (inputs, trivials, sample extracts, unpack bits, keyswitch results, bootstrap
 * results, results of another linear node; repeats allowed); creates M nodes of the operands' kind, all one level above the highest
 * operand, nodes_out[m] word-equal to row m of spf_lwe_linear_batch(slot, kind, B = 1) over those K rows in that order, bias
 * included.  The new nodes are ordinary: operands of any operation, outputs, counted by spf_graph_stats.  All layers of one level
 * with one (slot, M, K, operand kind) are one group: operand rows that lie consecutively in the graph's memory (the K results of
 * one bootstrap or keyswitch group, or of another layer) go to the dispatcher of spf_lwe_linear_enqueue in place, anything else is
 * ONE launch of lwe_linear_rows_kernel that reads the rows where they lie (the name spf_last_lwe_linear_kernel then gives; timed
 * as "lwe_linear").  A wrong argument (slot >= SPF_LWE_LINEAR_SLOTS, K = 0, M = 0 or M > SPF_GRAPH_LWE_LINEAR_MAX_ROWS, a null
 * pointer, a node that does not exist or is no LWE, lwe0 and lwe1 mixed) is SPF_ERR_INVALID_ARGUMENT from the call, nothing is
 * recorded and the graph stays usable.  The slot is read by spf_graph_run — it may be loaded after the graph is built, and loaded
 * again between runs under the rule of the key loads (the next run uses the new weights; a graph of a group reads the slot of the
 * member it runs on): before anything is enqueued, an empty slot is SPF_ERR_NO_KEY and a slot whose (M, K) is not the nodes' is
 * SPF_ERR_INVALID_ARGUMENT with both shapes in the message.
 * spf_lwe_linear_slot_shape: M, K and whether a bias is loaded in `slot`; SPF_ERR_NO_KEY while the slot is empty. */
typedef enum spf_graph_lwe_linear_limits { SPF_GRAPH_LWE_LINEAR_MAX_ROWS = 4096 } spf_graph_lwe_linear_limits;
spf_status spf_lwe_linear_slot_shape(spf_ctx *ctx, uint32_t slot, size_t *M, size_t *K, int *has_bias);
spf_status spf_graph_add_lwe_linear(spf_graph *graph, uint32_t slot, const uint32_t *lwe_nodes /* K */, size_t K,
                                    size_t M, uint32_t *nodes_out /* M */);
/* The plaintext polynomial linear map of polynomial weight slot `slot` (spf_load_glwe_poly_weights above) as a node constructor —
 * no FheOp there, no spf_graph_op here: a packed integer out of spf_graph_add_public_functional_keyswitch shifted and added to
 * another one before spf_graph_add_unpack, a lookup table that is a plaintext polynomial times an encrypted GLWE.
 * glwe_nodes[0 .. K) are glwe1 nodes of any origin and level (inputs, trivials, packs, CMUX and blind rotation results, results
 * of another such node; repeats allowed, within one list and across lists); creates M glwe1 nodes, all one level above the highest
 * operand, nodes_out[m] word-equal to row m of spf_glwe_poly_linear_batch(slot, B = 1) over those K GLWEs in that order, bias
 * included.  The new nodes are ordinary: operands of any operation, outputs, counted by spf_graph_stats.  All layers of one level
 * with one (slot, M, K) are one group and ONE launch: operands that lie consecutively in the graph's memory go to the kernels of
 * spf_glwe_poly_linear_enqueue in place, anything else to "glwe_poly_lds_rows_kernel" (or, on a constants-only slot,
 * "glwe_poly_stream_rows_kernel"; SPF_GLWE_POLY_PATH=lds forces the former), which read the GLWEs where they lie — the names
 * spf_last_glwe_poly_kernel then gives; timed as "glwe_poly_linear".  A wrong argument (a null pointer, slot >=
 * SPF_GLWE_POLY_SLOTS, K = 0 or K > 2^32 - 1, M = 0 or M > SPF_GLWE_POLY_MAX_ROWS, a node that does not exist or is no glwe1) is
 * SPF_ERR_INVALID_ARGUMENT from the call, nothing is recorded and the graph stays usable.  The slot is read by spf_graph_run — it
 * may be loaded after the graph is built, and loaded again between runs under the rule of the key loads (the next run uses the
 * new weights; a graph of a group reads the slot of the member it runs on): before anything is enqueued, an empty slot is
 * SPF_ERR_NO_KEY and a slot whose (M, K) is not the nodes' is SPF_ERR_INVALID_ARGUMENT with both shapes in the message. */
spf_status spf_graph_add_glwe_poly_linear(spf_graph *graph, uint32_t slot, const uint32_t *glwe_nodes /* K */, size_t K,
                                          size_t M, uint32_t *nodes_out /* M */);
/* The three operations of spf_glwe_keyswitch_* / spf_glwe_automorphism_* / spf_glwe_trace_* above as node constructors — no FheOp
 * there, no spf_graph_op here:
 *   spf_graph_add_glwe_keyswitch     `keyswitch_glwe_to_glwe` (sunscreen_tfhe/src/ops/fft_ops.rs:457-495; integer twin
 *                                    ops/keyswitch/glwe_keyswitch.rs:26-55) under the key in `slot`
 *   spf_graph_add_glwe_automorphism  one round of the trace's loop (`polynomial_pow_k`, ops/polynomial/mod.rs:62-84, then the
 *                                    keyswitch back: ops/automorphisms/mod.rs:72-83), `round` in 1 .. log2 N
 *   spf_graph_add_glwe_trace         `trace` (ops/automorphisms/mod.rs:53-85)
 * glwe_node is ONE glwe1 node of any origin (an input, a trivial constant, a CMUX or blind rotation result, a pack, a public
 * functional keyswitch, a row of a polynomial linear map, another of these nodes); each call creates one ordinary glwe1 node one
 * level above it, word-equal to the batch entry point at B = 1 over that GLWE: an operand of any operation that takes a glwe1, an
 * output, counted by spf_graph_stats.  A packed integer that changes its key, a GLWE traced behind an X^-j polynomial map to isolate
 * one coefficient, stay inside one spf_graph_run.  All such nodes of one level with one operation and one slot (or round) are one
 * group and ONE launch whatever their number: operands that lie consecutively in the graph's memory go to "glwe_ks_kernel" /
 * "generic_glwe_ks_kernel" in place, anything else to "glwe_ks_rows_kernel" / "generic_glwe_ks_rows_kernel", which read the GLWEs
 * where they lie through a pointer table (the same operand may stand in it several times) — the names
 * spf_last_glwe_keyswitch_kernel then gives; timed as "glwe_keyswitch".
 * SPF_ERR_INVALID_ARGUMENT from the call, with the offending numbers in the message, *node_out not written, nothing recorded and
 * the graph still usable: a null graph or node_out, glwe_node that is no node of the graph or no glwe1, slot >=
 * SPF_GLWE_KSK_SLOTS, round outside 1 .. log2 N.
 * Keys are read by spf_graph_run, before anything is enqueued and on the replay of a captured graph as well.  The keyswitch-key
 * slot may be loaded after the graph is built and loaded again between runs under the rule of the key loads: an empty slot is
 * SPF_ERR_NO_KEY, the next run after a load uses the new key (and the kernel its radix asks for); a load counts on the context,
 * and a captured graph (SPF_GRAPH_CAPTURE=1) that holds keyswitch nodes is dropped and captured anew when the count has moved.
 * Automorphism and trace nodes read the context's automorphism key at tr_radix: no key is SPF_ERR_NO_KEY, a tr_radix that no kernel
 * serves SPF_ERR_UNSUPPORTED with the text of the batch entry points.  spf_load_automorphism_key_* rewrites the key's one device
 * buffer in place, so a captured graph is KEPT over a reload and its replay reads the new key — what the circuit bootstrap nodes
 * of a captured graph do.  A graph of a group reads the keys of the member it runs on.
 * Not there yet: a row of the operation table, a lane of the pool, a submit by handle. */
spf_status spf_graph_add_glwe_keyswitch(spf_graph *graph, uint32_t slot, uint32_t glwe_node, uint32_t *node_out);
spf_status spf_graph_add_glwe_automorphism(spf_graph *graph, uint32_t round, uint32_t glwe_node, uint32_t *node_out);
spf_status spf_graph_add_glwe_trace(spf_graph *graph, uint32_t glwe_node, uint32_t *node_out);
/* FheOp::Output*: copy the node's value to `host` at the end of every run.  Plain (pageable) buffers: the run gathers every
 * output on the device and brings them back in ONE copy through the graph's own pinned staging (inputs go up the same way);
 * per-output copies to pageable memory cost ~20 us each on this runtime — 0.68 ms of a 32-bit addition's 5.5. */
spf_status spf_graph_add_output(spf_graph *graph, uint32_t node, void *host);
/* `run_graph_blocking`: returns when every output has been written */
spf_status spf_graph_run(spf_graph *graph);
/* nodes in the graph; levels and kernel launches of the most recent run */
spf_status spf_graph_stats(spf_graph *graph, uint32_t *nodes, uint32_t *levels, uint32_t *launches);

/* cmux over operands that are not contiguous: d_ptrs is a DEVICE array of 4 pointers per unit,
 * {selector GGSW-FFT, a (NULL = the zero ciphertext, i.e. multiply_glwe_ggsw), b, out}. */
spf_status spf_cmux_scattered_dev(spf_ctx *ctx, void *stream, size_t units, const void *const *d_ptrs);
/* dst row r = `words` u64 read from d_src_ptrs[r] (device array of device pointers) */
spf_status spf_gather_rows_dev(spf_ctx *ctx, void *stream, size_t rows, size_t words,
                               const uint64_t *const *d_src_ptrs, uint64_t *d_dst);

/* ---- ring packing: LWE or GLWE ciphertexts into one GLWE through the automorphism key ----
 * PackLWEs (Chen, Dai, Kim, Song): p = 2^m leaves per output, 1 <= p <= N, through p - 1 automorphism rounds in a tree of depth m
 * and the first log2 N - m rounds of the trace, under the automorphism key the circuit bootstrap already uses — no key of its own
 * (the public functional keyswitch, spf_public_functional_keyswitch_*, does the same job in n * L dependent rounds under a key of
 * 0.27 - 0.54 GB).  Not a function of the reference but a fixed composition of reference functions; with L = log2 N and
 * round(x, r) = keyswitch(x(X^t), ak[r-1]), t = N / 2^(r-1) + 1, the round of spf_glwe_automorphism_*:
 *   leaf   SPF_VAL_LWE1: g_j = the GLWE whose `sample_extract` at index 0 (ops/ciphertext/glwe_ciphertext_ops.rs:31-76) is leaf j and
 *          whose body coefficients 1 .. N-1 are 0; SPF_VAL_GLWE1: g_j = leaf j.  c_j^(0) = `polynomial_shr_round`(g_j, L) on every
 *          polynomial (the shift of `glwe_mod_switch_and_expand_pow_2`): the embedding first, the shift second.
 *   tree   for l = 1 .. m, cnt = p / 2^l, r = 0 .. cnt-1: E = c_r^(l-1), O = X^(N/2^l) * c_(r+cnt)^(l-1) (`mul_xn`),
 *          c_r^(l) = (E + O) + round(E - O, L - l + 1)                       (t = 2^l + 1)
 *   tail   x = c_0^(m); x <- x + round(x, r) for r = 1 .. L - m in turn: `trace` (ops/automorphisms/mod.rs:53-85) cut after L - m
 *          rounds.  p = N has no tail; p = 1 is the whole trace, what `mod_switch_trace_and_rotate` does to one level.
 * All additions wrap mod 2^64; the only floating-point step is the keyswitch, on exact input: every word equals the composition's.
 * LAYOUT: the result is STRIDED — the phase of coefficient j * N / p carries leaf j's message (as N * shr_round(., L) of it:
 * the message itself up to the L low bits the shift drops), every other coefficient carries 0.  This is not the packed integers'
 * "bit j at coefficient j" (spf_pack_*).  It is reached by spf_blind_rotation_* with log_stride = log2(N / p), by
 * spf_sample_extract_l1_each_* at the indices j * N / p, and by the polynomial linear maps (spf_glwe_poly_linear_*).
 * Leaves are [B][p] rows, output b's p leaves consecutive, of k*N+1 (SPF_VAL_LWE1) or (k+1)*N (SPF_VAL_GLWE1) words; the result
 * is B GLWEs of (k+1)*N words.
 * Launches: one per tree level over the nodes of all outputs, one for the tail: m + 1, m when p = N, 2 when p = 1 (the leaf's
 * conversion, then the trace).  N = 2048, k = 1 with tr_radix 6 levels x 7 bits runs the hand-written "ring_pack_kernel", every
 * other shape "generic_ring_pack_kernel" (spf_last_lwe_ring_pack_kernel); "lwe_ring_pack" of spf_last_kernel_ms has one entry per
 * launch.
 * Scratch: spf_lwe_ring_pack_scratch_words gives the words one call of B outputs needs (B * (p/2 + p/4) GLWEs, less for p <= 4).
 * spf_lwe_ring_pack_batch takes host pointers and owns its scratch: a call that would need more than 1 GiB runs in slices over B
 * (the environment variable SPF_LWE_RING_PACK_SCRATCH_BYTES, read at each call, overrides the cap: a testing knob).
 * spf_lwe_ring_pack_enqueue takes device pointers under the contract of the `_dev` entry points: it only enqueues on `stream`,
 * uses no buffer of the context, runs as ONE slice in the caller's scratch and leaves the scratch's contents undefined.
 * Statuses, decided before anything is queued, nothing touched: B = 0 is SPF_OK; no automorphism key is SPF_ERR_NO_KEY;
 * SPF_ERR_INVALID_ARGUMENT with the numbers in the message for p = 0, p not a power of two or p > N, a leaf kind other than
 * SPF_VAL_LWE1 / SPF_VAL_GLWE1, a scratch below the words needed, and any overlap of the output with the leaves or the scratch
 * (or of the scratch with the leaves).  The group form deals B in contiguous shards, an output's leaves with it. */
spf_status spf_lwe_ring_pack_batch(spf_ctx *ctx, spf_value_kind leaf_kind, size_t p, size_t B, const uint64_t *leaves, uint64_t *glwe_out);
spf_status spf_lwe_ring_pack_scratch_words(spf_ctx *ctx, size_t p, size_t B, size_t *words);
spf_status spf_lwe_ring_pack_enqueue(spf_ctx *ctx, void *stream, spf_value_kind leaf_kind, size_t p, size_t B, const uint64_t *d_leaves,
                                     uint64_t *d_scratch, size_t scratch_words, uint64_t *d_glwe_out);
const char *spf_last_lwe_ring_pack_kernel(spf_ctx *ctx);

/* ---- measurement hooks (bench.py) ------------------------------------------------------- */

/* Average device time in milliseconds of the launches of one kernel family made through this
 * context since timing was enabled (or since the last query, which clears the record), measured
 * with hipEvents recorded on the launch stream around each launch: "pbs" (blind rotation),
 * "keyswitch" (digits + GEMM), "trace" (cbs_trace_kernel), "scheme_switch", "cmux" (contiguous
 * batched CMUX family), "pufks_prepass" (the transposing pre-pass of a public functional keyswitch at the hand-written radices,
 * with the gather in front of it where there is one), "lwe_linear_planes" and "lwe_linear" (the per-call byte planes and the product,
 * with its bias, of spf_lwe_linear_enqueue; the VALU form records "lwe_linear" only), "glwe_poly_linear" (the one launch of spf_glwe_poly_linear_enqueue), "glwe_keyswitch" (the one launch of spf_glwe_keyswitch_enqueue, spf_glwe_automorphism_enqueue or spf_glwe_trace_enqueue), "lwe_ring_pack" (every launch of spf_lwe_ring_pack_enqueue: one entry per tree level, one for the tail).  A host-pointer bootstrap of more than one chip round is launched in slices
 * of 1024 ciphertexts: it records one "pbs" entry per slice.  Enable with spf_set_timing(ctx, 1). */
spf_status spf_set_timing(spf_ctx *ctx, int enabled);
spf_status spf_last_kernel_ms(spf_ctx *ctx, const char *kernel /* "pbs" | "keyswitch" | "trace" | "scheme_switch" | "cmux" | "pufks_prepass" | "lwe_linear_planes" | "lwe_linear" | "glwe_poly_linear" | "glwe_keyswitch" | "lwe_ring_pack" */,
                              double *avg_ms, int *launches);
/* `generate_lut` (sunscreen_tfhe ops/bootstrapping/programmable_bootstrapping.rs:129-185) for
 * `programmable_bootstrap_univariate`: map_tables[f * 2^bits + x] = f(x) for n_maps functions over a
 * plaintext space of 2^bits values (the reference takes closures; a table is their C form).  Writes the trivial
 * GLWE (zero mask, body = the rotated, half-negated table polynomial), (k+1)*N words.  No GPU involved; ctx-free.
 * A value >= 2^bits is SPF_ERR_INVALID_ARGUMENT (the reference asserts). */
spf_status spf_generate_lut(const spf_params *params, const uint64_t *map_tables, size_t n_maps,
                            uint32_t plaintext_bits, uint64_t *lut_glwe_out);
/* `BivariateLookupTable::trivial_from_fn` (sunscreen_tfhe entities/bivariate_lookup_table.rs:36-90) =
 * `generate_bivariate_lut` (ops/bootstrapping/programmable_bootstrapping.rs:413-452): map_table[l * 2^p + r] = f(l, r)
 * for p = plaintext_bits, 2^(2p) values.  Writes the trivial GLWE of `generate_lut` at p + carry_bits bits of the table
 * U[x] = f((x >> p) mod 2^p, x mod 2^p), x < 2^(p + carry_bits) (`bivariate_function`, :413-430: carry bits above 2p
 * are dropped), (k+1)*N words; outputs come out encoded at p + carry_bits bits without a padding bit
 * (`decrypt_lwe_with_carry`, high_level.rs:586-611).  Needs 1 <= p <= carry_bits, 2^(p + carry_bits) <= N and every
 * value < 2^p (the reference asserts), else SPF_ERR_INVALID_ARGUMENT.  No GPU involved; ctx-free. */
spf_status spf_generate_bivariate_lut(const spf_params *params, const uint64_t *map_table, uint32_t plaintext_bits,
                                      uint32_t carry_bits, uint64_t *lut_glwe_out);
/* `safe_bincode::deserialize::<ComputeKey>` + upload (parasol_runtime/src/safe_bincode.rs:16-28,
 * crypto/keys.rs:294-318): `bytes` is what the Rust side wrote with bincode DefaultOptions +
 * with_fixint_encoding — four sequences (u64 LE count, elements) in the order bs_key, ks_key, ss_key, auto_key.
 * Every count is checked against the context's parameters before anything is loaded; trailing bytes are allowed. */
spf_status spf_load_compute_key_bincode(spf_ctx *ctx, const uint8_t *bytes, size_t len);
/* `safe_bincode::deserialize::<ComputeKeyNonFft>` + `ComputeKeyNonFft::fft` + upload (crypto/keys.rs:145-159, :258-282): the
 * same bincode conventions, every element one little-endian u64, fields in the order of THAT struct — bs_key, ks_key, auto_key,
 * ss_key (not `ComputeKey`'s).  Every count is checked before anything is loaded; ks_key goes to spf_load_keyswitch_key, the
 * others to the `_std` loaders; trailing bytes are allowed. */
spf_status spf_load_compute_key_nonfft_bincode(spf_ctx *ctx, const uint8_t *bytes, size_t len);
/* Ciphertext wire format (parasol_runtime/src/crypto/encryption.rs:23-110: L0LweCiphertext, L1LweCiphertext,
 * L1GlweCiphertext, L1GlevCiphertext are serde newtypes over entities with one field `data: AVec<Torus<u64>>`,
 * sunscreen_tfhe/src/dst.rs:25-41) as `safe_bincode::deserialize` reads it (safe_bincode.rs:16-28): bincode
 * DefaultOptions + fixint encoding = a u64 little-endian element count, then the words little-endian; the read
 * is bounded by GetSize = (count + 1) * 8 bytes (encryption.rs:454-519), `check_is_valid` then demands exactly
 * the length the parameters give, trailing bytes are allowed.  L1GgswCiphertext is not Serialize in the
 * reference (encryption.rs:93-97): SPF_VAL_GGSW1 is SPF_ERR_UNSUPPORTED.  Host only, no GPU, ctx-free.
 *   spf_ciphertext_words:        number of u64 words of a ciphertext of `kind` (0 for an unknown kind)
 *   spf_ciphertext_from_bincode: bytes -> words_out (caller-allocated, spf_ciphertext_words(kind) words).  A count
 *                                that differs from the parameters' (the reference's malformed-length vector
 *                                safe_bincode.rs:58-66 included) or a truncated body is SPF_ERR_INVALID_ARGUMENT and
 *                                leaves words_out untouched.
 *   spf_ciphertext_to_bincode:   words -> out (capacity `cap` bytes); *written = 8 + 8 * words. */
size_t spf_ciphertext_words(const spf_params *params, spf_value_kind kind);
spf_status spf_ciphertext_from_bincode(const spf_params *params, spf_value_kind kind, const uint8_t *bytes, size_t len,
                                       uint64_t *words_out);
spf_status spf_ciphertext_to_bincode(const spf_params *params, spf_value_kind kind, const uint64_t *words, uint8_t *out,
                                     size_t cap, size_t *written);
/* `Evaluation::l1ggsw_zero()` / `l1ggsw_one()` (crypto/evaluation.rs:254-262): the GGSW (cbs radix, FFT domain,
 * (k+1)*l_cbs*(k+1)*N/2 complex) that `Evaluation::new` obtains by circuit-bootstrapping the trivial L0 LWE of
 * the bit (:161-197).  Computed on first use after the keys were (re)loaded, cached in HBM. */
spf_status spf_l1ggsw_constant(spf_ctx *ctx, int bit, double *ggsw_fft_out);
/* Device buffers for a caller that chains the `_dev` entry points but has no HIP binding of its own (the Rust shim of
 * INTEGRATION.md): hipMalloc / hipFree / hipMemcpy on the context's GPU.  `spf_device_download` first waits for everything
 * enqueued on `stream` (the stream the producing `_dev` call was given; NULL = the default stream), then copies.  No
 * reference counterpart (the reference keeps every ciphertext in host memory, crypto/encryption.rs:143-165). */
spf_status spf_device_alloc(spf_ctx *ctx, size_t bytes, void **dev_ptr);
spf_status spf_device_free(spf_ctx *ctx, void *dev_ptr);
spf_status spf_device_upload(spf_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
spf_status spf_device_download(spf_ctx *ctx, void *stream, void *host_dst, const void *dev_src, size_t bytes);
/* Name of the blind-rotation kernel the most recent bootstrap launch of this context used (the shape is
 * picked from the batch size: eight waves per ciphertext, two ciphertexts per workgroup, or the throughput
 * shape).  For measurement records; never NULL. */
const char *spf_last_blind_rotate_kernel(spf_ctx *ctx);
/* The same for the CMUX family (spf_cmux*, spf_glev_cmux*, spf_multiply_glwe_ggsw*, gate graphs): four waves per gate up
 * to one gate per CU, the streaming shape beyond, with streaming (non-temporal) selector loads once a launch's selectors
 * exceed the Infinity Cache.  The steps of spf_blind_rotation* report the same names with ",rot" appended
 * ("cmux4_kernel<4,4,rot>", "cmux_kernel<4,4,2,rot>", "cmux_kernel<4,4,2,stream,rot>"); the same step over scattered operands
 * (spf_graph_add_blind_rotation, spf_pool_submit_blind_rotation_v) appends ",scattered" ("cmux4_kernel<4,4,rot,scattered>",
 * "cmux_kernel<4,4,2,rot,scattered>"; generic contexts: "generic_cmux_rot_kernel").  Never NULL. */
const char *spf_last_cmux_kernel(spf_ctx *ctx);
/* The same for the LWE keyswitch L1 -> L0 (every entry point that runs one): "ks_gemm_lds_kernel", the int8 matrix-core
 * formulation, when the tuned context's radix fits it (radix_log <= 8 and its accumulator bound), else "keyswitch_kernel".
 * Never NULL. */
const char *spf_last_keyswitch_kernel(spf_ctx *ctx);
/* The same for spf_public_functional_keyswitch_* (public_functional_keyswitch.rs:74-148): on a tuned context at radix 4 bits x 8 or
 * 4 x 4 "pufks4_kernel<4,8>" / "pufks4_kernel<4,4>" (<LOGB,L>: four waves per output, one output per workgroup) up to one output per
 * CU, beyond that "pufks_kernel<4,8,G>" / "pufks_kernel<4,4,G>" (<LOGB,L,outputs per workgroup>), G = 2 while the call holds at
 * most two workgroups per CU, 4 beyond; a launch holds at most 4096 outputs (or what keeps its digits within 8 GiB), larger batches go in
 * several.  Everything else, N = 2048 / k = 1 at another radix included: "generic_pufks_kernel".  Never NULL. */
const char *spf_last_public_functional_keyswitch_kernel(spf_ctx *ctx);
/* The same for spf_private_functional_keyswitch_*, the components call and the circuit bootstrap via PFKS
 * (private_functional_keyswitch.rs:107-142): "pfks_gemm_kernel<U>" — the int8 matrix-core GEMM with U limbs per digit, U = 1 for
 * radix_log <= 8, else ceil((radix_log + 1) / 8): 2 up to 15 bits, 3 up to 23 — or "pfks_valu_kernel" for radix_log >= 24 and
 * for a key whose single tile of 128 rows of limbs would exceed the 1 GiB scratch cap of a launch.  A launch holds the rows whose
 * limbs fit that cap; larger batches go in several.  Never NULL. */
const char *spf_last_private_functional_keyswitch_kernel(spf_ctx *ctx);

/* ---- device groups: every GPU of a node from ONE host process (SURVEY.md §8 b / e) -------------------------------- *
 *
 * The caller being replaced is one process: `Evaluation` holds an `Arc<ComputeKey>` (crypto/evaluation.rs:144-197) and is
 * called from the rayon workers of one `CircuitProcessor` (circuit_processor/mod.rs:201-209).  A group is what that one
 * `Evaluation` owns on a multi-GPU node: one context per listed device (a device may be listed more than once: that many
 * contexts on it), the evaluation keys replicated INSIDE the library, and batch entry points that cut a host batch into
 * contiguous ranges of ceil(B / G) — bootstraps are independent units, there is no data-path collective — and drive every
 * member from its own host thread and stream.
 *
 * Keys: the loaders put the key on member 0 (host -> HBM) and replicate it: one RCCL communicator over the distinct
 * devices (`ncclCommInitAll`, single process) and an in-place `ncclBroadcast` of each key blob from member 0 over xGMI;
 * further members on an already served device take a device-to-device copy; every member then derives its own images
 * (keyswitch byte planes, scaled bootstrap key).  librccl.so is loaded on first use (dlopen); transport can be forced with
 * the environment variable SPF_GROUP_TRANSPORT = "rccl" (default whenever the group has more than one member; also taken
 * for a one-member group when set explicitly) or "peer" (hipMemcpyPeerAsync, no RCCL).  A transport NAMED there is never
 * replaced: a missing librccl.so with SPF_GROUP_TRANSPORT=rccl is SPF_ERR_HIP.  When rccl is only the default and librccl.so
 * cannot be loaded the group falls back to peer copies and says so (spf_group_replication_stats: transport
 * "peer (librccl.so could not be loaded)").
 *
 * Failures: a member whose call fails with SPF_ERR_HIP is taken out of rotation and its range is re-queued over the
 * remaining members ("a failed GPU's shard is re-queued by host"); the call fails only when no member is
 * left.  Any other status (invalid argument, missing key) is the caller's error and is returned at once.
 * `spf_group_set_member_enabled` drains or re-admits a device by hand.
 *
 * Thread safety: every entry point may be called from any number of host threads; calls are queued per member. */
typedef struct spf_group spf_group;
spf_status spf_group_create(const spf_params *params, const int *device_ids, int n_devices, spf_group **out);
void spf_group_destroy(spf_group *grp);
int spf_group_size(const spf_group *grp);
/* member i's context: for the `_dev` entry points, gate graphs and measurement hooks on that device.  Owned by the group:
 * never spf_destroy it; a pool or graph made on it keeps it alive past spf_group_destroy (Lifetimes, at spf_create). */
spf_ctx *spf_group_ctx(spf_group *grp, int member);
/* message of the last failing group call (storage of the calling thread, as spf_last_error) */
const char *spf_group_last_error(const spf_group *grp);

/* `ComputeKey` fields (crypto/keys.rs:306-318): upload to member 0, replicate, derive.  Same argument meaning as the
 * single-context loaders above. */
spf_status spf_group_load_bootstrap_key(spf_group *grp, const double *bsk_fft, size_t n_complex);
spf_status spf_group_load_keyswitch_key(spf_group *grp, const uint64_t *ksk, size_t n_words);
spf_status spf_group_load_automorphism_key(spf_group *grp, const double *ak_fft, size_t n_complex);
spf_status spf_group_load_scheme_switch_key(spf_group *grp, const double *ssk_fft, size_t n_complex);
spf_status spf_group_load_compute_key_bincode(spf_group *grp, const uint8_t *bytes, size_t len);
/* the standard (integer) forms (`ComputeKeyNonFft`, crypto/keys.rs:145-159, :258-282): member 0 transforms once, the spectra
 * are replicated as above — every member holds the same bits, the wire carries the same bytes as for the float loaders */
spf_status spf_group_load_bootstrap_key_std(spf_group *grp, const uint64_t *bsk, size_t n_words);
spf_status spf_group_load_automorphism_key_std(spf_group *grp, const uint64_t *ak, size_t n_words);
spf_status spf_group_load_scheme_switch_key_std(spf_group *grp, const uint64_t *ssk, size_t n_words);
spf_status spf_group_load_compute_key_nonfft_bincode(spf_group *grp, const uint8_t *bytes, size_t len);
/* `PublicFunctionalKeyswitchKey<u64>` (entities/public_functional_keyswitch_key.rs): as spf_load_public_functional_keyswitch_key_std */
spf_status spf_group_load_public_functional_keyswitch_key_std(spf_group *grp, const uint64_t *key, size_t n_words,
                                                              size_t from_dimension, uint32_t radix_log, uint32_t radix_count);
/* n_keys x `PrivateFunctionalKeyswitchKey<u64>` (entities/private_functional_keyswitch_key.rs:44-46): as
 * spf_load_private_functional_keyswitch_keys_std */
spf_status spf_group_load_private_functional_keyswitch_keys_std(spf_group *grp, const uint64_t *keys, size_t n_words, size_t n_keys,
                                                                size_t from_dimension, size_t lwe_count, uint32_t radix_log,
                                                                uint32_t radix_count);
/* replicate whatever member 0 holds (keys put there through spf_group_ctx(grp, 0), e.g. generated on the device into
 * spf_key_blob + spf_key_blob_commit) */
spf_status spf_group_replicate_keys(spf_group *grp);
/* totals since the group was created: seconds on the wire (communicator set-up counted separately), bytes received per
 * member, ranks of the RCCL communicator (0 = RCCL not used), transport name ("rccl", "peer", "none"; never NULL) */
spf_status spf_group_replication_stats(spf_group *grp, double *wire_seconds, double *comm_init_seconds, size_t *bytes_per_member,
                                       int *rccl_world_size, const char **transport);
/* take a member out of rotation (enabled = 0) or back in (1; also clears a recorded failure) */
spf_status spf_group_set_member_enabled(spf_group *grp, int member, int enabled);
/* members in rotation now */
int spf_group_members_in_rotation(spf_group *grp);
/* testing hook: the next `count` calls dispatched to `member` fail with SPF_ERR_HIP before touching the device */
spf_status spf_group_debug_fail_next(spf_group *grp, int member, int count);

/* The host-pointer batch forms over the group: same arguments as spf_*_batch, results word-identical to one context. */
spf_status spf_group_keyswitch_lwe_l1_lwe_l0_batch(spf_group *grp, size_t B, const uint64_t *lwe1_in, uint64_t *lwe0_out);
spf_status spf_group_generalized_pbs_batch(spf_group *grp, size_t B, const uint64_t *lwe0_in, const uint64_t *lut_glwe,
                                           size_t lut_stride, uint32_t log_chi, uint32_t log_v, uint64_t body_rotate,
                                           uint64_t *glwe_out);
spf_status spf_group_pbs_univariate_batch(spf_group *grp, size_t B, const uint64_t *lwe0_in, const uint64_t *lut_glwe,
                                          size_t lut_stride, uint64_t *lwe1_out);
spf_status spf_group_pbs_bivariate_batch(spf_group *grp, size_t B, const uint64_t *lwe0_left, const uint64_t *lwe0_right,
                                         const uint64_t *lut_glwe, size_t lut_stride, uint32_t plaintext_bits,
                                         uint64_t *lwe1_out);
spf_status spf_group_circuit_bootstrap_pbs_batch(spf_group *grp, size_t B, const uint64_t *lwe0_in, uint64_t *glwe_out);
spf_status spf_group_circuit_bootstrap_batch(spf_group *grp, size_t B, const uint64_t *lwe0_in, double *ggsw_fft_out);
spf_status spf_group_mod_switch_trace_and_rotate_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, uint64_t *glev_out);
spf_status spf_group_scheme_switch_batch(spf_group *grp, size_t B, const uint64_t *glev_in, double *ggsw_fft_out);
spf_status spf_group_sample_extract_l1_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, size_t idx, uint64_t *lwe1_out);
spf_status spf_group_glwe_not_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
spf_status spf_group_glwe_xor_batch(spf_group *grp, size_t B, const uint64_t *a, const uint64_t *b, uint64_t *glwe_out);
spf_status spf_group_glwe_mul_xn_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, size_t n, uint64_t *glwe_out);
spf_status spf_group_cmux_batch(spf_group *grp, size_t B, const double *sel_ggsw_fft, const uint64_t *a, const uint64_t *b,
                                uint64_t *out);
spf_status spf_group_glev_cmux_batch(spf_group *grp, size_t B, const double *sel_ggsw_fft, const uint64_t *a, const uint64_t *b,
                                     uint64_t *out);
spf_status spf_group_multiply_glwe_ggsw_batch(spf_group *grp, size_t B, const uint64_t *glwe, const double *ggsw_fft,
                                              uint64_t *out);
spf_status spf_group_gate_bootstrap_batch(spf_group *grp, size_t B, const uint64_t *lwe1_in, uint64_t *glwe_out);
spf_status spf_group_keyswitch_circuit_bootstrap_batch(spf_group *grp, size_t B, const uint64_t *lwe1_in, double *ggsw_fft_out);
/* the packed-integer forms, sharded by packed ciphertext (a member's rows are at * n_bits onwards) */
spf_status spf_group_glwe_pack_batch(spf_group *grp, size_t B, size_t n_bits, const uint64_t *bits_glwe, uint64_t *packed_out);
spf_status spf_group_glwe_unpack_l1_batch(spf_group *grp, size_t B, size_t n_bits, const uint64_t *packed_glwe,
                                          uint64_t *lwe1_out);
spf_status spf_group_unpack_circuit_bootstrap_batch(spf_group *grp, size_t B, size_t n_bits, const uint64_t *packed_glwe,
                                                    double *ggsw_fft_out);
/* `blind_rotation` (ops/bootstrapping/blind_rotation.rs:202-223), sharded by item (a member's selectors are at * n_bits onwards) */
spf_status spf_group_blind_rotation_batch(spf_group *grp, size_t B, size_t n_bits, size_t log_stride, const double *shift_ggsw_fft,
                                          const uint64_t *glwe_in, uint64_t *glwe_out);
/* `public_functional_keyswitch` (ops/keyswitch/public_functional_keyswitch.rs:74-148), sharded by output (a member's rows are
 * at * lwe_count onwards) */
spf_status spf_group_public_functional_keyswitch_batch(spf_group *grp, size_t B, size_t lwe_count, const uint64_t *lwe_in,
                                                       uint64_t *glwe_out);
/* `private_functional_keyswitch` (ops/keyswitch/private_functional_keyswitch.rs:107-142), sharded by output (a member's rows are
 * at * lwe_count onwards), and `circuit_bootstrap_via_pfks` (ops/bootstrapping/circuit_bootstrapping.rs:162-219), sharded by item */
spf_status spf_group_private_functional_keyswitch_batch(spf_group *grp, size_t key_index, size_t B, const uint64_t *lwe_in,
                                                        uint64_t *glwe_out);
spf_status spf_group_circuit_bootstrap_via_pfks_batch(spf_group *grp, size_t B, const uint64_t *lwe0_in, double *ggsw_fft_out);
/* the plaintext linear maps (`scalar_mul_ciphertext_mad` + `add_lwe_inplace`, ops/ciphertext/lwe_ciphertext_ops.rs:48-66, :4-18;
 * spf_load_lwe_linear_weights, spf_lwe_linear_batch): the weights go to every member, straight from the host pointer; a batch is
 * sharded by input vector (a member's K ciphertexts are at * K onwards) */
spf_status spf_group_load_lwe_linear_weights(spf_group *grp, uint32_t slot, size_t M, size_t K, const int64_t *weights,
                                             const uint64_t *bias);
spf_status spf_group_lwe_linear_batch(spf_group *grp, uint32_t slot, spf_value_kind kind, size_t B, const uint64_t *lwe_in,
                                      uint64_t *lwe_out);
/* the plaintext polynomial linear maps over GLWE ciphertexts (`glwe_polynomial_mad` and its kin, ops/ciphertext/
 * glwe_ciphertext_ops.rs:164-183; spf_load_glwe_poly_weights, spf_glwe_poly_linear_batch): the weights go to every member,
 * straight from the host pointers; a batch is sharded by item (a member's K GLWEs are at * K onwards) */
spf_status spf_group_load_glwe_poly_weights(spf_group *grp, uint32_t slot, size_t M, size_t K, const uint32_t *offsets,
                                            const uint32_t *exponents, const int64_t *coefficients, const uint64_t *bias);
spf_status spf_group_glwe_poly_linear_batch(spf_group *grp, uint32_t slot, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
/* GLWE keyswitch, one automorphism round and the trace (`keyswitch_glwe_to_glwe`, ops/fft_ops.rs:457-495; ops/automorphisms/
 * mod.rs:53-85; spf_load_glwe_keyswitch_key_std, spf_glwe_keyswitch_batch, spf_glwe_automorphism_batch, spf_glwe_trace_batch): the
 * key goes to every member, straight from the host pointer; a batch is sharded by item */
spf_status spf_group_load_glwe_keyswitch_key_std(spf_group *grp, uint32_t slot, const uint64_t *key, size_t n_words,
                                                 uint32_t radix_log, uint32_t radix_count);
spf_status spf_group_glwe_keyswitch_batch(spf_group *grp, uint32_t slot, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
spf_status spf_group_glwe_automorphism_batch(spf_group *grp, uint32_t round, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
spf_status spf_group_glwe_trace_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, uint64_t *glwe_out);
/* ring packing (spf_lwe_ring_pack_batch): the automorphism key is the members' own; a batch is sharded by output, an output's p
 * leaves go with it */
spf_status spf_group_lwe_ring_pack_batch(spf_group *grp, spf_value_kind leaf_kind, size_t p, size_t B, const uint64_t *leaves,
                                         uint64_t *glwe_out);
/* The per-item forms (spf_sample_extract_l1_each_batch, spf_glwe_mul_xn_each_batch, spf_glwe_keyswitch_each_batch,
 * spf_glwe_automorphism_each_batch): a batch is sharded by item and the parameter array is dealt in the same contiguous shards;
 * the checks are made on the whole batch before any member is touched */
spf_status spf_group_sample_extract_l1_each_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, const uint64_t *idx,
                                                  uint64_t *lwe1_out);
spf_status spf_group_glwe_mul_xn_each_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, const uint64_t *amounts,
                                            uint64_t *glwe_out);
spf_status spf_group_glwe_keyswitch_each_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, const uint64_t *slots,
                                               uint64_t *glwe_out);
spf_status spf_group_glwe_automorphism_each_batch(spf_group *grp, size_t B, const uint64_t *glwe_in, const uint64_t *rounds,
                                                  uint64_t *glwe_out);
/* `Evaluation::l1ggsw_zero` / `l1ggsw_one` (identical on every member: same keys, same kernels; taken from member 0) */
spf_status spf_group_l1ggsw_constant(spf_group *grp, int bit, double *ggsw_fft_out);

/* Gate-graph jobs over the group — `CircuitProcessor::run_graph_blocking` for a POOL of independent circuits on a multi-GPU node
 * (circuit_processor/mod.rs:573-623; the multiplier circuits of circuits/mul.rs:90-200; BASELINE config 5).  The unit dealt to a
 * device is the job (one graph): cutting one graph across GPUs would ship a 256 KiB GGSW per selector crossing the cut,
 * independent graphs need nothing.
 *   spf_group_graph_create: a graph that is not bound to a device yet; built with spf_graph_add_* as usual (same validation).
 *   spf_group_run_graphs:   deals the n jobs over the members in rotation by cost, longest processing time first (cost =
 *       50 x circuit bootstraps + other operations of the job; ties by position: deterministic), lowers every member's jobs
 *       into ONE graph on its device — the level-batching executor then sees K jobs x gates per level — runs the members side
 *       by side on their worker threads and returns when every output of every job has been written.  The merged graphs are
 *       kept while the same jobs come again (new input contents, same DAGs).  A member that fails with SPF_ERR_HIP leaves the
 *       rotation and its jobs are dealt again over the others.  Results are word-identical to spf_graph_run of each job on one
 *       context.  spf_graph_run / spf_graph_stats / spf_graph_destroy work on such a graph (run = a pool of one; stats = of
 *       the job as built: levels and launches are those of the merged graph it last ran in).
 *   spf_graph_member:       the member a group's graph last ran on (-1 before its first run; 0 for an ordinary graph).
 * A job retains its group until spf_graph_destroy (Lifetimes, at spf_create). */
spf_status spf_group_graph_create(spf_group *grp, spf_graph **out);
spf_status spf_group_run_graphs(spf_group *grp, spf_graph *const *graphs, size_t n);
int spf_graph_member(const spf_graph *graph);

/* Call coalescing over the group: one pool per member; a calling thread is dealt to a member on its first submit
 * (round-robin over the members in rotation) and stays there, so that the callers of one device keep coming back to the
 * same batch.  The handle is used with the spf_pool_submit_*, spf_pool_wait, spf_pool_stats (sums), spf_pool_set_max_inflight
 * (per member) and spf_pool_destroy entry points above.  The pool retains the group until spf_pool_destroy (Lifetimes, at spf_create). */
spf_status spf_pool_create_group(spf_group *grp, size_t max_batch, uint32_t max_wait_us, spf_pool **out);

/* Library / kernel build information: version, target, the compile-time options of the blind rotation. */
const char *spf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPF_HIP_H */
