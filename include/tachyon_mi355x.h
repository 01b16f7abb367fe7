/*
 * tachyon_mi355x.h -- C-ABI of the MI355X MSM + NTT backend.
 *
 * The entry points in the "reference C-ABI" sections keep the names, argument
 * meaning, ownership and error behaviour of Tachyon's tachyon/c API
 * (reference snapshot /root/reference, cited per declaration) so a binary
 * linked against libtachyon.so's MSM / univariate-domain symbols can link
 * against libtachyon_mi355x.so instead.  Entry points prefixed
 * tachyon_mi355x_ are extensions (device-resident buffers, G2 MSM, multi-GPU
 * helpers, synthetic inputs, timings); they have no reference counterpart.
 *
 * Data layout (identical to the reference, msm_input_provider.h:23-29
 * bit-casts these structs to its native types):
 *   field elements: Montgomery form, R = 2^(64*N), little-endian 64-bit limbs
 *   affine / point2: {x, y}, identity = (0, 0) (affine_point.h:39,125)
 *   jacobian / projective: {x, y, z};  xyzz: {x, y, zz, zzz}
 *
 * Ownership: returned points / containers are allocated with C++ operator
 * new (as msm.h:45 / msm_gpu.h:81 / bn254_univariate_evaluation_domain.cc:50-85
 * do); free them with delete (C++) or the matching *_destroy / free helper.
 * Errors: like the reference's CHECK, any failure prints a message and aborts.
 * There is no CPU fallback: every compute entry point needs a HIP device.
 */
#ifndef TACHYON_MI355X_H_
#define TACHYON_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#define TACHYON_C_EXPORT __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

/* ---- field and point types (prime_field.h.tpl / point.h.tpl:22-94) -------- */
typedef struct tachyon_bn254_fq { uint64_t limbs[4]; } tachyon_bn254_fq;
typedef struct tachyon_bn254_fr { uint64_t limbs[4]; } tachyon_bn254_fr;
typedef struct tachyon_bn254_fq2 { tachyon_bn254_fq c0, c1; } tachyon_bn254_fq2;
typedef struct tachyon_bls12_381_fq { uint64_t limbs[6]; } tachyon_bls12_381_fq;
typedef struct tachyon_bls12_381_fr { uint64_t limbs[4]; } tachyon_bls12_381_fr;
typedef struct tachyon_bls12_381_fq2 { tachyon_bls12_381_fq c0, c1; } tachyon_bls12_381_fq2;

#define TACHYON_MI355X_POINT_TYPES(C, G, F)                                   \
  typedef struct tachyon_##C##_##G##_affine { F x, y; } tachyon_##C##_##G##_affine;             \
  typedef struct tachyon_##C##_##G##_point2 { F x, y; } tachyon_##C##_##G##_point2;             \
  typedef struct tachyon_##C##_##G##_jacobian { F x, y, z; } tachyon_##C##_##G##_jacobian;      \
  typedef struct tachyon_##C##_##G##_projective { F x, y, z; } tachyon_##C##_##G##_projective;  \
  typedef struct tachyon_##C##_##G##_xyzz { F x, y, zz, zzz; } tachyon_##C##_##G##_xyzz;

TACHYON_MI355X_POINT_TYPES(bn254, g1, tachyon_bn254_fq)
TACHYON_MI355X_POINT_TYPES(bn254, g2, tachyon_bn254_fq2)
TACHYON_MI355X_POINT_TYPES(bls12_381, g1, tachyon_bls12_381_fq)
TACHYON_MI355X_POINT_TYPES(bls12_381, g2, tachyon_bls12_381_fq2)
#undef TACHYON_MI355X_POINT_TYPES

/* ========================================================================== */
/* Reference C-ABI: MSM (generated per curve from                              */
/* tachyon/c/math/elliptic_curves/generator/msm{,_gpu}.h.tpl; G1 only there)   */
/* ========================================================================== */
typedef struct tachyon_bn254_g1_msm* tachyon_bn254_g1_msm_ptr;               /* msm.h.tpl:21 */
typedef struct tachyon_bn254_g1_msm_gpu* tachyon_bn254_g1_msm_gpu_ptr;       /* msm_gpu.h.tpl:17 */
typedef struct tachyon_bls12_381_g1_msm* tachyon_bls12_381_g1_msm_ptr;
typedef struct tachyon_bls12_381_g1_msm_gpu* tachyon_bls12_381_g1_msm_gpu_ptr;

/* point.cc.tpl:7-9 -- curve constant initialisation; constants are compiled in here, so a no-op. */
TACHYON_C_EXPORT void tachyon_bn254_g1_init(void);
TACHYON_C_EXPORT void tachyon_bls12_381_g1_init(void);
TACHYON_C_EXPORT void tachyon_bn254_g2_init(void);
TACHYON_C_EXPORT void tachyon_bls12_381_g2_init(void);

/* msm.h.tpl:30-58 (CPU-named entry points; served by the MI355X backend). */
TACHYON_C_EXPORT tachyon_bn254_g1_msm_ptr tachyon_bn254_g1_create_msm(uint8_t degree);
TACHYON_C_EXPORT void tachyon_bn254_g1_destroy_msm(tachyon_bn254_g1_msm_ptr ptr);
TACHYON_C_EXPORT tachyon_bn254_g1_jacobian* tachyon_bn254_g1_point2_msm(
    tachyon_bn254_g1_msm_ptr ptr, const tachyon_bn254_g1_point2* bases, const tachyon_bn254_fr* scalars,
    size_t size);
TACHYON_C_EXPORT tachyon_bn254_g1_jacobian* tachyon_bn254_g1_affine_msm(
    tachyon_bn254_g1_msm_ptr ptr, const tachyon_bn254_g1_affine* bases, const tachyon_bn254_fr* scalars,
    size_t size);

/* msm_gpu.h.tpl:26-54 -> tachyon/c/math/elliptic_curves/msm/msm_gpu.h:23-122. */
TACHYON_C_EXPORT tachyon_bn254_g1_msm_gpu_ptr tachyon_bn254_g1_create_msm_gpu(uint8_t degree);
TACHYON_C_EXPORT void tachyon_bn254_g1_destroy_msm_gpu(tachyon_bn254_g1_msm_gpu_ptr ptr);
TACHYON_C_EXPORT tachyon_bn254_g1_jacobian* tachyon_bn254_g1_point2_msm_gpu(
    tachyon_bn254_g1_msm_gpu_ptr ptr, const tachyon_bn254_g1_point2* bases, const tachyon_bn254_fr* scalars,
    size_t size);
TACHYON_C_EXPORT tachyon_bn254_g1_jacobian* tachyon_bn254_g1_affine_msm_gpu(
    tachyon_bn254_g1_msm_gpu_ptr ptr, const tachyon_bn254_g1_affine* bases, const tachyon_bn254_fr* scalars,
    size_t size);

TACHYON_C_EXPORT tachyon_bls12_381_g1_msm_ptr tachyon_bls12_381_g1_create_msm(uint8_t degree);
TACHYON_C_EXPORT void tachyon_bls12_381_g1_destroy_msm(tachyon_bls12_381_g1_msm_ptr ptr);
TACHYON_C_EXPORT tachyon_bls12_381_g1_jacobian* tachyon_bls12_381_g1_point2_msm(
    tachyon_bls12_381_g1_msm_ptr ptr, const tachyon_bls12_381_g1_point2* bases,
    const tachyon_bls12_381_fr* scalars, size_t size);
TACHYON_C_EXPORT tachyon_bls12_381_g1_jacobian* tachyon_bls12_381_g1_affine_msm(
    tachyon_bls12_381_g1_msm_ptr ptr, const tachyon_bls12_381_g1_affine* bases,
    const tachyon_bls12_381_fr* scalars, size_t size);
TACHYON_C_EXPORT tachyon_bls12_381_g1_msm_gpu_ptr tachyon_bls12_381_g1_create_msm_gpu(uint8_t degree);
TACHYON_C_EXPORT void tachyon_bls12_381_g1_destroy_msm_gpu(tachyon_bls12_381_g1_msm_gpu_ptr ptr);
TACHYON_C_EXPORT tachyon_bls12_381_g1_jacobian* tachyon_bls12_381_g1_point2_msm_gpu(
    tachyon_bls12_381_g1_msm_gpu_ptr ptr, const tachyon_bls12_381_g1_point2* bases,
    const tachyon_bls12_381_fr* scalars, size_t size);
TACHYON_C_EXPORT tachyon_bls12_381_g1_jacobian* tachyon_bls12_381_g1_affine_msm_gpu(
    tachyon_bls12_381_g1_msm_gpu_ptr ptr, const tachyon_bls12_381_g1_affine* bases,
    const tachyon_bls12_381_fr* scalars, size_t size);

/* ========================================================================== */
/* Reference C-ABI: univariate evaluation domain over BN254 Fr                 */
/* (tachyon/c/math/polynomials/univariate/bn254_univariate_*.h)               */
/* ========================================================================== */
typedef struct tachyon_bn254_univariate_evaluation_domain tachyon_bn254_univariate_evaluation_domain;
typedef struct tachyon_bn254_univariate_evaluations tachyon_bn254_univariate_evaluations;
typedef struct tachyon_bn254_univariate_dense_polynomial tachyon_bn254_univariate_dense_polynomial;
typedef struct tachyon_bn254_univariate_rational_evaluations tachyon_bn254_univariate_rational_evaluations;

/* bn254_univariate_evaluation_domain.h:38-136 */
TACHYON_C_EXPORT tachyon_bn254_univariate_evaluation_domain* tachyon_bn254_univariate_evaluation_domain_create(
    size_t num_coeffs);
TACHYON_C_EXPORT void tachyon_bn254_univariate_evaluation_domain_destroy(
    tachyon_bn254_univariate_evaluation_domain* domain);
TACHYON_C_EXPORT tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluation_domain_empty_evals(
    const tachyon_bn254_univariate_evaluation_domain* domain);
TACHYON_C_EXPORT tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_evaluation_domain_empty_poly(
    const tachyon_bn254_univariate_evaluation_domain* domain);
/* size() rational zeros 0/1 (bn254_univariate_evaluation_domain.h:70-79) */
TACHYON_C_EXPORT tachyon_bn254_univariate_rational_evaluations*
tachyon_bn254_univariate_evaluation_domain_empty_rational_evals(const tachyon_bn254_univariate_evaluation_domain* domain);
TACHYON_C_EXPORT tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluation_domain_fft(
    const tachyon_bn254_univariate_evaluation_domain* domain, const tachyon_bn254_univariate_dense_polynomial* poly);
TACHYON_C_EXPORT tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluation_domain_fft_inplace(
    const tachyon_bn254_univariate_evaluation_domain* domain, tachyon_bn254_univariate_dense_polynomial* poly);
TACHYON_C_EXPORT tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_evaluation_domain_ifft(
    const tachyon_bn254_univariate_evaluation_domain* domain, const tachyon_bn254_univariate_evaluations* evals);
TACHYON_C_EXPORT tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_evaluation_domain_ifft_inplace(
    const tachyon_bn254_univariate_evaluation_domain* domain, tachyon_bn254_univariate_evaluations* evals);

/* bn254_univariate_evaluations.h:36-79 */
TACHYON_C_EXPORT tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluations_create(void);
TACHYON_C_EXPORT tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluations_clone(
    const tachyon_bn254_univariate_evaluations* evals);
TACHYON_C_EXPORT void tachyon_bn254_univariate_evaluations_destroy(tachyon_bn254_univariate_evaluations* evals);
TACHYON_C_EXPORT size_t tachyon_bn254_univariate_evaluations_len(const tachyon_bn254_univariate_evaluations* evals);
TACHYON_C_EXPORT void tachyon_bn254_univariate_evaluations_set_value(tachyon_bn254_univariate_evaluations* evals,
                                                                     size_t i, const tachyon_bn254_fr* value);

/* bn254_univariate_rational_evaluations.h: UnivariateEvaluations<RationalField<bn254::Fr>>
 * (numerator / denominator pairs, zero = 0/1; boundary checks are the caller's).
 * _evaluate: numerator / denominator of element i (aborts on a zero
 * denominator, like RationalField::Evaluate's unwrap); _batch_evaluate: a new
 * evaluations container of every quotient, zero where the denominator is zero
 * (RationalField::BatchEvaluate + DoBatchInverse, groups.h:124-180), computed
 * on the GPU (Montgomery's batch-inversion trick). */
TACHYON_C_EXPORT tachyon_bn254_univariate_rational_evaluations* tachyon_bn254_univariate_rational_evaluations_create(
    void);
TACHYON_C_EXPORT tachyon_bn254_univariate_rational_evaluations* tachyon_bn254_univariate_rational_evaluations_clone(
    const tachyon_bn254_univariate_rational_evaluations* evals);
TACHYON_C_EXPORT void tachyon_bn254_univariate_rational_evaluations_destroy(
    tachyon_bn254_univariate_rational_evaluations* evals);
TACHYON_C_EXPORT size_t tachyon_bn254_univariate_rational_evaluations_len(
    const tachyon_bn254_univariate_rational_evaluations* evals);
TACHYON_C_EXPORT void tachyon_bn254_univariate_rational_evaluations_set_zero(
    tachyon_bn254_univariate_rational_evaluations* evals, size_t i);
TACHYON_C_EXPORT void tachyon_bn254_univariate_rational_evaluations_set_trivial(
    tachyon_bn254_univariate_rational_evaluations* evals, size_t i, const tachyon_bn254_fr* numerator);
TACHYON_C_EXPORT void tachyon_bn254_univariate_rational_evaluations_set_rational(
    tachyon_bn254_univariate_rational_evaluations* evals, size_t i, const tachyon_bn254_fr* numerator,
    const tachyon_bn254_fr* denominator);
TACHYON_C_EXPORT void tachyon_bn254_univariate_rational_evaluations_evaluate(
    const tachyon_bn254_univariate_rational_evaluations* evals, size_t i, tachyon_bn254_fr* value);
TACHYON_C_EXPORT tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_rational_evaluations_batch_evaluate(
    const tachyon_bn254_univariate_rational_evaluations* evals);

/* bn254_univariate_dense_polynomial.h (create/clone/destroy) */
TACHYON_C_EXPORT tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_dense_polynomial_create(void);
TACHYON_C_EXPORT tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_dense_polynomial_clone(
    const tachyon_bn254_univariate_dense_polynomial* poly);
TACHYON_C_EXPORT void tachyon_bn254_univariate_dense_polynomial_destroy(
    tachyon_bn254_univariate_dense_polynomial* poly);

/* ========================================================================== */
/* Extensions (no reference counterpart)                                       */
/* ========================================================================== */
/* Container access the reference performs through C++ native_cast. */
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_evaluations_get_value(
    const tachyon_bn254_univariate_evaluations* evals, size_t i, tachyon_bn254_fr* value);
TACHYON_C_EXPORT tachyon_bn254_fr* tachyon_mi355x_bn254_univariate_evaluations_data(
    tachyon_bn254_univariate_evaluations* evals);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_evaluations_resize(tachyon_bn254_univariate_evaluations* evals,
                                                                         size_t len);
TACHYON_C_EXPORT size_t tachyon_mi355x_bn254_univariate_dense_polynomial_len(
    const tachyon_bn254_univariate_dense_polynomial* poly);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_dense_polynomial_resize(
    tachyon_bn254_univariate_dense_polynomial* poly, size_t len);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_dense_polynomial_set_value(
    tachyon_bn254_univariate_dense_polynomial* poly, size_t i, const tachyon_bn254_fr* value);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_dense_polynomial_get_value(
    const tachyon_bn254_univariate_dense_polynomial* poly, size_t i, tachyon_bn254_fr* value);
TACHYON_C_EXPORT tachyon_bn254_fr* tachyon_mi355x_bn254_univariate_dense_polynomial_data(
    tachyon_bn254_univariate_dense_polynomial* poly);

/* rational container access the reference performs through native_cast */
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_rational_evaluations_resize(
    tachyon_bn254_univariate_rational_evaluations* evals, size_t len);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_rational_evaluations_get(
    const tachyon_bn254_univariate_rational_evaluations* evals, size_t i, tachyon_bn254_fr* numerator,
    tachyon_bn254_fr* denominator);

/* halo2 BN254 Fr generator set (math::halo2, bn/bn254/halo2/bn254.h:9-17):
 * _override = OverrideSubgroupGenerator() (bn254.cc:7-30: generator 7 and
 * halo2curves' two-adic / large-subgroup roots of unity), _restore = the
 * ScopedSubgroupGeneratorOverrider destructor (bn254.cc:40-44, back to the
 * arkworks-compatible generator 5).  Process-wide; domains, four-step plans
 * and KZG setups created afterwards use the active set (Domain::Create
 * captures the root).  _active returns 1 while the halo2 set is installed. */
TACHYON_C_EXPORT void tachyon_mi355x_bn254_halo2_override_subgroup_generator(void);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_halo2_restore_subgroup_generator(void);
TACHYON_C_EXPORT int tachyon_mi355x_bn254_halo2_subgroup_generator_active(void);

/* Domain queries and the coset hook (UnivariateEvaluationDomain::GetCoset,
 * univariate_evaluation_domain.h:102-117): set_offset turns the domain into
 * its coset h*<w>; offset 1 restores it. */
TACHYON_C_EXPORT size_t tachyon_mi355x_bn254_univariate_evaluation_domain_size(
    const tachyon_bn254_univariate_evaluation_domain* domain);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_evaluation_domain_group_gen(
    const tachyon_bn254_univariate_evaluation_domain* domain, tachyon_bn254_fr* out);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_evaluation_domain_set_offset(
    tachyon_bn254_univariate_evaluation_domain* domain, const tachyon_bn254_fr* offset);
/* Device-resident in-place transform of size() elements at d_data (HBM),
 * enqueued on the domain's stream (see _stream).  inverse = 0: FFT,
 * 1: IFFT (no trimming).  Not synchronised.  _batch_device transforms `batch`
 * consecutive arrays of size() elements. */
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_evaluation_domain_transform_device(
    tachyon_bn254_univariate_evaluation_domain* domain, tachyon_bn254_fr* d_data, int inverse);
/* Host-resident in-place transform (IcicleNTT<bn254::Fr>::Run on a host
 * pointer, icicle_ntt.h:53-142 / icicle_ntt_bn254.cc:31-116: natural order in
 * and out, the domain's coset offset): inout holds exactly size() Montgomery
 * elements; synchronous.  The C++ hook over it is
 * include/tachyon_mi355x_ntt_holder.h (IcicleNTTHolder's shape). */
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_evaluation_domain_transform_host(
    tachyon_bn254_univariate_evaluation_domain* domain, tachyon_bn254_fr* inout, size_t len, int inverse);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_evaluation_domain_transform_batch_device(
    tachyon_bn254_univariate_evaluation_domain* domain, tachyon_bn254_fr* d_data, size_t batch, int inverse);
TACHYON_C_EXPORT void* tachyon_mi355x_bn254_univariate_evaluation_domain_stream(
    tachyon_bn254_univariate_evaluation_domain* domain);
/* per-pass device time (ms) of the last transform when profiling is on;
 * returns the number of passes written. */
TACHYON_C_EXPORT void tachyon_mi355x_bn254_univariate_evaluation_domain_set_profile(
    tachyon_bn254_univariate_evaluation_domain* domain, int on);
/* Kernel variant of the domain's transforms (no reference counterpart):
 * 0 = the 8 x 32-bit-limb passes, 1 = the 9 x 29-bit-limb passes, 3 = the
 * 29-bit passes with XOR-swizzled LDS positions; a new domain uses 1 up to
 * 2^20 elements and 0 above (the faster of the two at each size).  All compute
 * the same canonical outputs.  Returns 0 (nothing changed) for other values. */
TACHYON_C_EXPORT int tachyon_mi355x_bn254_univariate_evaluation_domain_set_variant(
    tachyon_bn254_univariate_evaluation_domain* domain, int variant);
/* One process, several GPUs: later transforms of the plain domain (offset 1;
 * a coset keeps the single device) through the fft/ifft entry points above,
 * transform_host and transform_device run the four-step NTT over `count`
 * devices (ids may repeat: logical devices sharing a GPU) -- part g on ids[g],
 * the all-to-all as peer copies over xGMI, input and output in natural order
 * on the device the domain was created on (transform_device: a buffer there).
 * The four-step splits by a power of two: the first 2^k ids are used, the
 * largest 2^k <= count with 2^k <= 2^floor(log n / 2) (_devices reports
 * them); count <= 1 restores the single device, and so does 2^k = 2: two
 * parts exchange n/4 elements over ONE xGMI link, which takes longer than
 * the whole transform on one MI355X (2^24: 134 MB at <= 153 GB/s >= 0.9 ms
 * plus 2 x 0.55 ms of local stages, against 1.84 ms) -- from four parts the
 * all-to-all spreads over 3+ links and the split pays.  Returns 1, or 0 (nothing
 * changed) for a bad id, a domain too small for two parts, or when the
 * generator set active now differs from the domain's (the plans would use
 * another root).  Same results as one device. */
TACHYON_C_EXPORT int tachyon_mi355x_bn254_univariate_evaluation_domain_set_devices(
    tachyon_bn254_univariate_evaluation_domain* domain, const int* ids, size_t count);
/* the device list of set_devices (0 = single device); writes up to cap ids */
TACHYON_C_EXPORT size_t tachyon_mi355x_bn254_univariate_evaluation_domain_devices(
    const tachyon_bn254_univariate_evaluation_domain* domain, int* ids, size_t cap);
TACHYON_C_EXPORT int tachyon_mi355x_bn254_univariate_evaluation_domain_last_timings(
    const tachyon_bn254_univariate_evaluation_domain* domain, float* total_ms, float* pass_ms, int max_passes);

/* Distributed four-step NTT over 2^log_world ranks (no
 * reference counterpart -- icicle's NTT is single-GPU).  One plan per rank;
 * rank r holds the columns c in [r C/G, (r+1) C/G) of the R x C view of the
 * input (R = 2^floor(log_n/2)), column-major: in[c_l R + r'] = x[C r' + c],
 * and produces rows k1 in [r R/G, (r+1) R/G) of the output, row-major:
 * out[k1_l C + k2] = X[k1 + R k2].  A transform is
 *   stage(1, in -> send); all-to-all(send -> recv) by the caller; stage(2, recv -> out)
 * with send/recv = G chunks of local_size/G elements (chunk h to/from rank h).
 * The inverse maps the output layout back to the input layout (n^-1 included).
 *
 * Ordering contract.  Every stage is enqueued on the plan's stream (`stream`
 * at create, a hipStream_t; NULL = a non-blocking stream the plan owns;
 * _stream returns it) and returns without synchronising.  The stages wait for
 * nothing else: the caller (1) makes the plan's stream wait for whatever
 * produced d_in (hipEventRecord on the producer + hipStreamWaitEvent, or
 * produce it on the plan's stream), (2) runs its all-to-all on the plan's
 * stream -- e.g. ncclAllToAll / RCCL with that stream -- or orders it after
 * stage 1 with an event, and (3) does the same before reading d_out.  A
 * non-blocking stream does not order against the legacy NULL stream, so
 * "same stream" must be meant literally.  tachyon_amd.dist.sharded_ntt keeps
 * the contract (tests/test_gpu_dist.py produces the input on another stream). */
typedef struct tachyon_mi355x_bn254_ntt4 tachyon_mi355x_bn254_ntt4;
TACHYON_C_EXPORT tachyon_mi355x_bn254_ntt4* tachyon_mi355x_bn254_ntt4_create(uint32_t log_n, uint32_t log_world,
                                                                            uint32_t rank, void* stream);
/* The same plan with R = 2^log_r (1 <= log_r < log_n, R and C = n / R >= G):
 * the layouts above with that R.  _split_log_r returns the split with the
 * fewest pass launches (passes of <= 8 stages; ties: the larger R up to C),
 * e.g. 2^24 -> R = 2^8, C = 2^16: one pass for the column NTTs (several
 * columns per workgroup) and two for the rows, against 2 + 2 for 2^12 x 2^12.
 * _log_rows returns a plan's log R. */
TACHYON_C_EXPORT tachyon_mi355x_bn254_ntt4* tachyon_mi355x_bn254_ntt4_create_split(uint32_t log_n, uint32_t log_r,
                                                                                  uint32_t log_world, uint32_t rank,
                                                                                  void* stream);
TACHYON_C_EXPORT uint32_t tachyon_mi355x_bn254_ntt4_log_rows(const tachyon_mi355x_bn254_ntt4* plan);
TACHYON_C_EXPORT uint32_t tachyon_mi355x_ntt4_split_log_r(uint32_t log_n, uint32_t log_world);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_ntt4_destroy(tachyon_mi355x_bn254_ntt4* plan);
TACHYON_C_EXPORT size_t tachyon_mi355x_bn254_ntt4_local_size(const tachyon_mi355x_bn254_ntt4* plan);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_ntt4_stage(tachyon_mi355x_bn254_ntt4* plan, int stage, int inverse,
                                                      const tachyon_bn254_fr* d_in, tachyon_bn254_fr* d_out);
TACHYON_C_EXPORT void tachyon_mi355x_bn254_ntt4_synchronize(tachyon_mi355x_bn254_ntt4* plan);
TACHYON_C_EXPORT void* tachyon_mi355x_bn254_ntt4_stream(const tachyon_mi355x_bn254_ntt4* plan);
/* A/B (every variant gives the same bytes): bit 0 = the round-4 stages (an
 * input copy, the passes, a separate twiddle kernel) instead of the exchange's
 * twiddle and packing fused into the sub-transforms' passes; bit 1 = the
 * sub-transforms on the 8 x 32-bit-limb passes instead of their size's
 * default (29-bit up to 2^20); bit 2 = one column per workgroup in one-pass
 * sub-transforms (no packing); bit 3 = the exchange twiddles computed in the
 * pass instead of read from the plan's precomputed table.  Returns 0 for other
 * values. */
TACHYON_C_EXPORT int tachyon_mi355x_bn254_ntt4_set_variant(tachyon_mi355x_bn254_ntt4* plan, int variant);

/* ---- field-generic radix-2 NTT domains --------------------------------------
 * Radix2EvaluationDomain<F> FFT / IFFT on the GPU for the scalar fields the
 * reference's icicle backend covers: field 1 = bn254 Fr (IcicleNTT<bn254::Fr>,
 * icicle_ntt_bn254.cc:31-116), 3 = bls12_381 Fr (IcicleNTT<bls12_381::Fr>,
 * icicle_ntt_bls12_381.cc:31-115).  Elements are the field's 4 x uint64
 * Montgomery limbs (tachyon_bn254_fr / tachyon_bls12_381_fr).  size =
 * bit_ceil(num_coeffs); the root is the field's two-adic root squared down
 * (bn254 Fr: the generator set active at creation, halo2 override included).
 * _set_offset: the coset h * <w> of later transforms (NULL or 1 = the plain
 * domain; GetCoset, univariate_evaluation_domain.h:102-117).
 * _transform_host: IcicleNTT::Run -- in place on a host vector of exactly
 * size() elements, natural order, forward (coefficients -> evaluations) or
 * inverse (n^-1 and the coset included); synchronous.  _transform_device:
 * `batch` consecutive device arrays in place, enqueued on _stream.  Returns
 * NULL from _create for another field id; failures abort. */
typedef struct tachyon_mi355x_ntt_domain tachyon_mi355x_ntt_domain;
TACHYON_C_EXPORT tachyon_mi355x_ntt_domain* tachyon_mi355x_ntt_domain_create(int field, size_t num_coeffs);
TACHYON_C_EXPORT void tachyon_mi355x_ntt_domain_destroy(tachyon_mi355x_ntt_domain* d);
TACHYON_C_EXPORT size_t tachyon_mi355x_ntt_domain_size(const tachyon_mi355x_ntt_domain* d);
TACHYON_C_EXPORT int tachyon_mi355x_ntt_domain_field(const tachyon_mi355x_ntt_domain* d);
TACHYON_C_EXPORT void tachyon_mi355x_ntt_domain_group_gen(const tachyon_mi355x_ntt_domain* d, void* out);
TACHYON_C_EXPORT void tachyon_mi355x_ntt_domain_set_offset(tachyon_mi355x_ntt_domain* d, const void* offset);
TACHYON_C_EXPORT void tachyon_mi355x_ntt_domain_transform_host(tachyon_mi355x_ntt_domain* d, void* inout, size_t len,
                                                              int inverse);
TACHYON_C_EXPORT void tachyon_mi355x_ntt_domain_transform_device(tachyon_mi355x_ntt_domain* d, void* d_data,
                                                                size_t batch, int inverse);
TACHYON_C_EXPORT void* tachyon_mi355x_ntt_domain_stream(tachyon_mi355x_ntt_domain* d);

/* The drop-in IcicleNTT engine (icicle_ntt.h:43-87, icicle_ntt_bn254.cc:31-101,
 * icicle_ntt_holder.h:30-44): a holder created without a size, initialised
 * once from a generator of order 2^LN, then serving FFT / IFFT of every
 * power-of-two size <= 2^LN (w_size = group_gen^(2^LN / size)) on any coset --
 * one holder for domain_ and extended_domain_ (zk/base/entities/entity.h:83-95).
 * field: 1 bn254 Fr, 3 bls12_381 Fr, 4 baby_bear (below; NULL for another id); stream: a
 * hipStream_t, or NULL for a stream the handle owns.  Single device (the
 * current one).  Every int-returning call returns 1 on success and 0 on
 * refusal; nothing aborts, and a refused _run leaves inout untouched.
 *   _init: group_gen_mont (32 bytes, Montgomery) must have order exactly
 *     2^LN, 0 <= LN <= min(two-adicity, 30).  options (NULL: the defaults
 *     below): batch_size >= 1, columns_batch == 0, ordering == 0 (natural to
 *     natural), are_inputs_on_device == are_outputs_on_device;
 *     fast_twiddles_mode is ignored.  On an initialised handle: 1 for the same
 *     generator (nothing changes), 0 for another.
 *   _run: in place on batch_size contiguous transforms of `size` elements
 *     (Montgomery form, natural order in and out), size a power of two in
 *     [1, 2^LN].  coset_canonical: 32 little-endian bytes, canonical form
 *     (F::ToBigInt()), 1 = no coset; 0 and values >= the modulus are refused.
 *     algorithm (0 Auto, 1 Radix2, 2 MixedRadix) does not change the result.
 *     Host data: copied in and out, synchronised.  Device data: on _stream,
 *     synchronised unless is_async; coset tables are built on the device and
 *     the last 8 (size, coset) pairs are kept.
 *   _release frees the tables (then _run refuses and _init works again);
 *   _log_order: LN, or -1 when not initialised; _table_bytes: device bytes of
 *   the stage, 29-bit and cached coset tables. */
typedef struct tachyon_mi355x_icicle_ntt tachyon_mi355x_icicle_ntt;
typedef struct {
  int fast_twiddles_mode;    /* default 1 */
  int batch_size;            /* default 1 */
  int columns_batch;         /* default 0 */
  int ordering;              /* default 0 = kNN */
  int are_inputs_on_device;  /* default 0 */
  int are_outputs_on_device; /* default 0 */
  int is_async;              /* default 0 */
} tachyon_mi355x_icicle_ntt_options;
TACHYON_C_EXPORT tachyon_mi355x_icicle_ntt* tachyon_mi355x_icicle_ntt_create(int field, void* stream);
TACHYON_C_EXPORT int tachyon_mi355x_icicle_ntt_init(tachyon_mi355x_icicle_ntt* h, const void* group_gen_mont,
                                                    const tachyon_mi355x_icicle_ntt_options* options);
TACHYON_C_EXPORT int tachyon_mi355x_icicle_ntt_run(tachyon_mi355x_icicle_ntt* h, int algorithm,
                                                   const void* coset_canonical, void* inout, size_t size,
                                                   int inverse);
TACHYON_C_EXPORT int tachyon_mi355x_icicle_ntt_release(tachyon_mi355x_icicle_ntt* h);
TACHYON_C_EXPORT void tachyon_mi355x_icicle_ntt_destroy(tachyon_mi355x_icicle_ntt* h);
TACHYON_C_EXPORT int tachyon_mi355x_icicle_ntt_log_order(const tachyon_mi355x_icicle_ntt* h);
TACHYON_C_EXPORT void* tachyon_mi355x_icicle_ntt_stream(tachyon_mi355x_icicle_ntt* h);
TACHYON_C_EXPORT size_t tachyon_mi355x_icicle_ntt_table_bytes(const tachyon_mi355x_icicle_ntt* h);

/* Field 4 = baby_bear (IcicleNTT<BabyBear>, icicle_ntt_baby_bear.cc:31-115;
 * p = 2^31 - 2^27 + 1, one uint32 Montgomery word with R = 2^32) for the
 * tachyon_mi355x_icicle_ntt_* entries only (tachyon_mi355x_ntt_domain_create(4)
 * stays NULL).  As documented above, except:
 *   elements and group_gen_mont are 4 bytes (group_gen_mont < p), LN <= 27;
 *   coset_canonical is 8 little-endian bytes (the reference's BigInt<1>) with
 *     a value in [1, p): 0, values >= p and any bit above 32 are refused;
 *   columns_batch may be 1: _run then treats inout as a size x batch_size
 *     row-major matrix and transforms every column;
 *   the passes index with 32 bits: size * batch_size, rows * cols and
 *     (rows << added_bits) * cols must be below 2^32, anything larger is refused;
 *   _table_bytes: the two-level twiddle tables and the cached coset tables
 *     (96 KiB per base, under 1 MiB in all, at LN = 27; no table grows with 2^LN / 2).
 * The two entries below are valid for field 4 only and return 0 for a handle
 * of another field.
 *   _run_matrix: Radix2EvaluationDomain::FFTBatch (radix2_evaluation_domain.h:
 *     99-127) and its inverse: in place on every column of a rows x cols
 *     row-major matrix (element (i, c) at i * cols + c), rows a power of two in
 *     [1, 2^LN], cols >= 1; the handle's batch_size / columns_batch are
 *     ignored, its residency and is_async apply.
 *   _coset_lde_batch: CosetLDEBatch with reverse_at_last
 *     (radix2_evaluation_domain.h:129-197, naive_batch_fft.h:68-121).  Per
 *     column: the inverse transform at `rows` on the plain domain, coefficient
 *     j times shift^j / rows, zero padding to rows << added_bits, the forward
 *     transform at that size; natural order.  `in` (rows x cols) is not
 *     written, `out` holds (rows << added_bits) x cols.  Refused: rows not a
 *     power of two, rows << added_bits above 2^LN, cols == 0, a shift (8
 *     bytes, canonical) outside [1, p), in == out with added_bits > 0
 *     (added_bits == 0 in place is allowed).
 *   _last_launches: kernel launches of the last transform on the handle. */
TACHYON_C_EXPORT int tachyon_mi355x_icicle_ntt_run_matrix(tachyon_mi355x_icicle_ntt* h, int algorithm,
                                                          const void* coset_canonical, void* inout, size_t rows,
                                                          size_t cols, int inverse);
TACHYON_C_EXPORT int tachyon_mi355x_icicle_ntt_coset_lde_batch(tachyon_mi355x_icicle_ntt* h, const void* in,
                                                               size_t rows, size_t cols, size_t added_bits,
                                                               const void* shift_canonical, void* out);
TACHYON_C_EXPORT unsigned tachyon_mi355x_icicle_ntt_last_launches(const tachyon_mi355x_icicle_ntt* h);

/* ---- Poseidon2 over BabyBear and FieldMerkleTree<BabyBear, 8> ---------------
 * The hash side of TwoAdicFRI::Commit (two_adic_fri.h:76-94 ->
 * FieldMerkleTreeMMCS::CommitOwned): Poseidon2 of width 16, x^7, 8 full and 13
 * partial rounds (Poseidon2Params<BabyBear, 15, 7>, Grain LFSR constants, the
 * Plonky3 internal layer with shifts), PaddingFreeSponge<., 8, 8> leaf hashes,
 * TruncatedPermutation<., 8, 2> compression, FieldMerkleTree::Build with mixed
 * heights, bytewise the reference's results.  Elements are 4-byte Montgomery
 * words as for field 4 above; a BabyBear4 matrix is the base-field matrix with
 * 4 x the columns.  external_matrix picks the 4 x 4 block of the external
 * layer: 0 Horizen (5 7 1 3 / 4 6 1 1 / 1 3 5 7 / 1 1 4 6), 1 Plonky3 (the
 * circulant 2 3 1 1).  Nothing aborts: 1 = success, 0 = refusal.
 *
 *   _permute: `count` states of 16 words in place.  Host states are copied
 *     both ways and the call returns when they are back; device states are
 *     enqueued on `stream` (waited for only when stream is NULL).
 *   _create / _destroy: a tree on `stream` (NULL: a stream of its own).
 *   _build: `count` row-major matrices, matrix m rows[m] x cols[m] words, host
 *     or device memory each (hipPointerGetAttributes).  Host matrices are
 *     uploaded and kept; device matrices are referenced, not copied: the
 *     caller keeps them alive and unchanged for _open.  With device matrices
 *     the call only enqueues on the tree's stream.  Matrices are stable-sorted
 *     by height, descending; the tallest ones are hashed row by row
 *     (concatenated in that order) into layer 0, padded with zero digests to
 *     bit_ceil(rows); a later layer of size s takes the matrices with
 *     bit_ceil(rows) == s as next[i] = C(C(prev[2i], prev[2i+1]), H(row i)),
 *     the zero digest in place of H for rows <= i < s.
 *     flags: TACHYON_MI355X_MERKLE_BIT_REVERSED makes leaf i of every matrix its
 *     stored row bitrev(i) over log2(rows) bits: committing the natural-order
 *     output of _icicle_ntt_coset_lde_batch with it gives the layers the
 *     reference gets from its bit-reversed LDE, without a permuted copy.
 *     Refused, the tree keeping what it held: null pointers, count 0, rows or
 *     cols 0, unknown flags, heights that round up to the same power of two
 *     but differ, the flag with a height that is not a power of two, more than
 *     16 matrices in one layer, rows above 2^30, a row above 2^24 words.
 *     Also 0 on a HIP error; if the layer buffer cannot be allocated the tree
 *     is left without a build (_num_layers 0).
 *   _num_layers: log2(bit_ceil(max rows)) + 1, 0 before a build.
 *     _layer_size(k): digests in layer k.  _layer / _root: copies of 8-word
 *     digests to host memory (they wait for the stream); a layer is the
 *     reference's std::vector<std::array<F, 8>>.  _layers_device_ptr: the
 *     layers one after another in device memory, layer 0 first.
 *   _open (DoCreateOpeningProof): rows_out[m] receives cols[m] words, row
 *     index >> (log_max - ceil_log2(rows[m])) of matrix m in the caller's order
 *     (mapped through bitrev with the flag; zeros when that row is past the
 *     height of a matrix whose height is no power of two); siblings_out
 *     receives num_layers - 1 digests, layer[k][(index >> k) ^ 1].  Refused:
 *     no tree built, index >= _layer_size(0), null pointers.
 *   _last_launches: kernel launches of the last _build.
 *   tachyon_mi355x_baby_bear_mul_rate: Montgomery products per second of
 *     `iters` rounds of 4 chained in-register products in `threads` lanes (the
 *     VALU yardstick of tools/poseidon2_probe.py); 0 on failure. */
#define TACHYON_MI355X_POSEIDON2_HORIZEN 0
#define TACHYON_MI355X_POSEIDON2_PLONKY3 1
#define TACHYON_MI355X_MERKLE_BIT_REVERSED 1u
typedef struct tachyon_mi355x_baby_bear_merkle_tree tachyon_mi355x_baby_bear_merkle_tree;
TACHYON_C_EXPORT int tachyon_mi355x_poseidon2_baby_bear_permute(int external_matrix, void* states, size_t count,
                                                                void* stream);
TACHYON_C_EXPORT tachyon_mi355x_baby_bear_merkle_tree* tachyon_mi355x_baby_bear_merkle_tree_create(
    int external_matrix, void* stream);
TACHYON_C_EXPORT void tachyon_mi355x_baby_bear_merkle_tree_destroy(tachyon_mi355x_baby_bear_merkle_tree* tree);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_merkle_tree_build(tachyon_mi355x_baby_bear_merkle_tree* tree,
                                                                const void* const* matrices, const size_t* rows,
                                                                const size_t* cols, size_t count, unsigned flags);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_merkle_tree_root(tachyon_mi355x_baby_bear_merkle_tree* tree, void* out);
TACHYON_C_EXPORT size_t tachyon_mi355x_baby_bear_merkle_tree_num_layers(
    const tachyon_mi355x_baby_bear_merkle_tree* tree);
TACHYON_C_EXPORT size_t tachyon_mi355x_baby_bear_merkle_tree_layer_size(
    const tachyon_mi355x_baby_bear_merkle_tree* tree, size_t k);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_merkle_tree_layer(tachyon_mi355x_baby_bear_merkle_tree* tree, size_t k,
                                                                void* out);
TACHYON_C_EXPORT const void* tachyon_mi355x_baby_bear_merkle_tree_layers_device_ptr(
    const tachyon_mi355x_baby_bear_merkle_tree* tree);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_merkle_tree_open(tachyon_mi355x_baby_bear_merkle_tree* tree,
                                                               size_t index, void* const* rows_out,
                                                               void* siblings_out);
TACHYON_C_EXPORT unsigned tachyon_mi355x_baby_bear_merkle_tree_last_launches(
    const tachyon_mi355x_baby_bear_merkle_tree* tree);
TACHYON_C_EXPORT void* tachyon_mi355x_baby_bear_merkle_tree_stream(tachyon_mi355x_baby_bear_merkle_tree* tree);
TACHYON_C_EXPORT double tachyon_mi355x_baby_bear_mul_rate(size_t threads, unsigned iters);

/* ---- BabyBear4 and the FRI opening ------------------------------------------
 * TwoAdicFRI::CreateOpeningProof (two_adic_fri.h:96-219, prove.h,
 * fri_config.h) without its challenger: the caller's transcript samples alpha
 * and every beta and hands them in; each commit-phase root is handed back
 * before the next beta is needed.  A BabyBear4 element is 4 Montgomery words
 * c0..c3 of F[x] / (x^4 - 11), 16 bytes.  Every result is a canonical element,
 * bytewise the reference's.  1 = success, 0 = refusal; a refusal leaves the
 * handle as it was, except the zero-denominator one.
 *
 *   tachyon_mi355x_baby_bear4_ops: out[i] = a[i] op b[i] on `count` elements,
 *     op 0 add, 1 sub, 2 mul, 3 square, 4 inverse (b is ignored by 3 and 4 and
 *     may be NULL; the inverse of 0 is 0).  All arrays host memory (copied both
 *     ways, the call returns when `out` is written) or all device memory
 *     (enqueued on `stream`, waited for only when stream is NULL); out may be a
 *     or b.  Refused: unknown op, null pointers, count 0 or above 2^28, host
 *     and device memory mixed.
 *   _create(log_blowup, external_matrix, stream) / _destroy: log_blowup 1..26,
 *     external_matrix as for the tree; stream NULL: a stream of its own.
 *   _begin(alpha): forgets everything and sets the batching challenge (4
 *     canonical Montgomery words; like every element handed in, at any 4-byte
 *     alignment).
 *   _add_round: one commit round's `count` extensions in the order of the
 *     round's tree, matrix m rows[m] x cols[m] words in natural row order on
 *     the coset 31 <w_rows> (what _icicle_ntt_coset_lde_batch wrote), host or
 *     device memory each; device matrices are referenced until the next _begin.
 *     points[m]: num_points[m] BabyBear4 opening points in host memory;
 *     opened_values_out[m]: num_points[m] * cols[m] elements of host memory,
 *     the values of point p at [p * cols[m] ..) (both may be NULL for a matrix
 *     without points, which still creates its height's zero input).  Adds
 *     alpha^offset (rr[i] - sum_c alpha^c ys[c]) / (x_i - z) to the reduced
 *     opening of the matrix's height, offsets running across matrices, points
 *     and rounds in the reference's order.  Waits for the stream once.
 *     Refused: null pointers, count 0, cols 0 or above 2^24, rows no power of
 *     two, below 2^log_blowup or above 2^27, a non-canonical point, a call
 *     before _begin or after the first _commit.  A point inside 31 <w_rows>
 *     (where the reference CHECKs) is found on the device: the call returns 0
 *     and the handle refuses everything until the next _begin.
 *   _num_inputs / _input_log_size(k) / _input(k, out) / _input_device_ptr(k):
 *     the reduced openings, largest first, 2^log_size elements each in the
 *     reference's (bit-reversed) order: position i belongs to natural row
 *     bitrev(i).  _input copies to host memory and waits.
 *   _commit(root_out): while the folded vector is longer than 2^log_blowup,
 *     builds a FieldMerkleTree over it as size/2 rows of 8 words, copies the
 *     8-word root to root_out (waits once) and returns 1; returns 0 once the
 *     phase has ended.  The first call freezes the inputs.  Refused (0 as
 *     well): no input, a root that _fold has not consumed yet.
 *   _fold(beta): FoldMatrix with the challenge sampled after that root, plus
 *     the input of the new size if there is one.  Only enqueues.  Refused:
 *     no pending _commit, a non-canonical beta.
 *   _num_commits: trees built so far.  _final_poly(out): the last 2^log_blowup
 *     values (all equal for honest inputs; final_eval is the first), after the
 *     phase has ended.
 *   _answer_query(index, sibling_values_out, siblings_out) (AnswerQuery): for
 *     commit-phase tree i, sibling_values_out[i] is element (index >> i) ^ 1 of
 *     that step's vector, and siblings_out receives the log_max - i - 1 digests
 *     of leaf (index >> i) >> 1, tree 0 first, each from the leaf layer up.
 *     Refused: before the phase has ended, index >= the largest input's size.
 *   _last_launches: kernel launches of the last _add_round, _commit, _fold or
 *     _answer_query.  _stream: the stream everything is enqueued on. */
typedef struct tachyon_mi355x_baby_bear_fri_opening tachyon_mi355x_baby_bear_fri_opening;
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear4_ops(int op, const void* a, const void* b, void* out, size_t count,
                                                   void* stream);
TACHYON_C_EXPORT tachyon_mi355x_baby_bear_fri_opening* tachyon_mi355x_baby_bear_fri_opening_create(
    unsigned log_blowup, int external_matrix, void* stream);
TACHYON_C_EXPORT void tachyon_mi355x_baby_bear_fri_opening_destroy(tachyon_mi355x_baby_bear_fri_opening* h);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_opening_begin(tachyon_mi355x_baby_bear_fri_opening* h,
                                                                const void* alpha);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_opening_add_round(
    tachyon_mi355x_baby_bear_fri_opening* h, const void* const* ldes, const size_t* rows, const size_t* cols,
    size_t count, const void* const* points, const size_t* num_points, void* const* opened_values_out);
TACHYON_C_EXPORT size_t tachyon_mi355x_baby_bear_fri_opening_num_inputs(const tachyon_mi355x_baby_bear_fri_opening* h);
TACHYON_C_EXPORT unsigned tachyon_mi355x_baby_bear_fri_opening_input_log_size(
    const tachyon_mi355x_baby_bear_fri_opening* h, size_t k);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_opening_input(tachyon_mi355x_baby_bear_fri_opening* h, size_t k,
                                                                void* out);
TACHYON_C_EXPORT const void* tachyon_mi355x_baby_bear_fri_opening_input_device_ptr(
    const tachyon_mi355x_baby_bear_fri_opening* h, size_t k);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_opening_commit(tachyon_mi355x_baby_bear_fri_opening* h,
                                                                 void* root_out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_opening_fold(tachyon_mi355x_baby_bear_fri_opening* h,
                                                               const void* beta);
TACHYON_C_EXPORT size_t tachyon_mi355x_baby_bear_fri_opening_num_commits(
    const tachyon_mi355x_baby_bear_fri_opening* h);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_opening_final_poly(tachyon_mi355x_baby_bear_fri_opening* h,
                                                                     void* out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_opening_answer_query(tachyon_mi355x_baby_bear_fri_opening* h,
                                                                       size_t index, void* sibling_values_out,
                                                                       void* siblings_out);
TACHYON_C_EXPORT unsigned tachyon_mi355x_baby_bear_fri_opening_last_launches(
    const tachyon_mi355x_baby_bear_fri_opening* h);
TACHYON_C_EXPORT void* tachyon_mi355x_baby_bear_fri_opening_stream(tachyon_mi355x_baby_bear_fri_opening* h);

/* ---- DuplexChallenger, grinding and the opening proof in one call ------------
 * DuplexChallenger<Poseidon2, 16, R> over BabyBear (duplex_challenger.h:33-65,
 * challenger.h:54-127), Challenger::Grind on the GPU, the openings of a tree
 * and the queries of an opening at many indices at once, and
 * TwoAdicFRI::CreateOpeningProof followed by fri::Prove (two_adic_fri.h:96-219,
 * prove.h:121-159) as one call.  Words are Montgomery words; 1 = success, 0 or
 * NULL = refusal, and a refusal leaves the handles as they were.
 *
 * The challenger is host code: everything but _grind / _grind_range works
 * without a GPU.  The permutation is the device one, bytewise.
 *   _create(external_matrix, rate): a zero state and empty buffers; rate 1..16
 *     words absorbed per permutation (SP1 8).  _clone: an independent copy.
 *   _observe(values, count) (DoObserve): each word clears the output buffer and
 *     joins the input buffer, which is duplexed at once when it holds `rate`
 *     words.  Refused, nothing observed: a word >= p, null pointers.
 *   _sample(out, count) (DoSample): duplexes first when there are inputs or no
 *     outputs, then pops from the back of the output buffer (the 16 state
 *     words).  _sample_ext(out): 4 samples, c0 first (SampleExtElement).
 *   _sample_bits(bits, out): FromMontgomery(sample) & (2^bits - 1).  Refused
 *     without sampling: bits above 30 (the reference requires 2^bits < p).
 *   _check_witness(bits, witness) (CheckWitness): observes the witness, samples
 *     the bits and returns 1 when they are 0.  The transcript advances either
 *     way, as the reference's does; bits above 30 or a witness >= p return 0
 *     and leave it where it was.
 *   _state(out): 50 words: the 16 state words, the length of the input buffer
 *     and its words in 16 slots, the length of the output buffer and its words
 *     in 16 slots (unused slots 0).
 *   _grind(bits, witness_out, stream) / _grind_range(bits, from, to, ...)
 *     (Grind, challenger.h:87-122): the SMALLEST canonical w in [from, to), [0,
 *     p) without a range, with CheckWitness(bits, w), as a Montgomery word; the
 *     challenger is left as that CheckWitness leaves it.  The reference returns
 *     the first hit of its first thread chunk that has one, which depends on
 *     its thread count; on one thread it is this value.  The search runs on
 *     the GPU in ascending chunks, one launch, one copy-back and one wait
 *     each, and stops after the first chunk with a hit.  Refused, the
 *     challenger unchanged: bits above 30, from >= to, to > p, null pointers, no
 *     witness in the range (the reference CHECKs).
 *
 *   tachyon_mi355x_baby_bear_merkle_tree_open_batch(tree, indices, count,
 *     rows_out, siblings_out): _open at `count` indices.  rows_out[m] receives
 *     count x cols[m] words and siblings_out count x (num_layers - 1) digests,
 *     query q's part what _open(indices[q]) writes.  One gather launch, one
 *     copy per output array, one wait.
 *   tachyon_mi355x_baby_bear_fri_opening_answer_queries(h, indices, count,
 *     sibling_values_out, siblings_out): _answer_query at `count` indices, query
 *     q's part in _answer_query's layout at q times its size.  One launch, two
 *     copies, one wait.
 *   Both refuse, writing nothing: null pointers, count 0 or above 2^16, any
 *     index the single call refuses.
 *
 *   _fri_opening_prove(h, challenger, rounds, num_rounds, num_queries,
 *     proof_of_work_bits): a round is its commit's tree, built with
 *     TACHYON_MI355X_MERKLE_BIT_REVERSED over device-resident natural-order
 *     extensions that it still references, and _add_round's points, num_points
 *     and opened_values_out for the tree's matrices in its order.  The
 *     transcript: alpha = SampleExtElement; _begin and _add_round per round
 *     (the opened values go to the caller, who observes them afterwards, as in
 *     the reference); per commit-phase step the root is observed and beta
 *     sampled; final_eval is observed; the witness is ground on the GPU;
 *     num_queries x SampleBits(log_max); one _answer_queries; one _open_batch
 *     per round tree at index >> (log_max - the tree's log height).  Refused
 *     with NULL, the challenger and the opening unchanged: null pointers,
 *     num_rounds 0, num_queries 0 or above 2^16, bits above 30, a tree not
 *     built or built without the flag, a tree or a challenger of another
 *     external matrix than the opening's, whatever _add_round refuses.  A point
 *     inside the coset returns NULL with the challenger restored and the
 *     opening needing a new _begin.
 *   _fri_proof_*: _num_commits / _commits(out) (8 words each), _final_eval(out)
 *     (4 words), _pow_witness(out) (1 word), _num_queries / _query_index(q),
 *     _query_steps(q, sibling_values_out, siblings_out) in _answer_query's
 *     layout, _query_input(q, round, rows_out, siblings_out) in _open's layout,
 *     _destroy.  Refused: null pointers, q or round out of range. */
typedef struct tachyon_mi355x_baby_bear_duplex_challenger tachyon_mi355x_baby_bear_duplex_challenger;
typedef struct tachyon_mi355x_baby_bear_fri_proof tachyon_mi355x_baby_bear_fri_proof;
typedef struct {
  tachyon_mi355x_baby_bear_merkle_tree* tree;
  const void* const* points;
  const size_t* num_points;
  void* const* opened_values_out;
} tachyon_mi355x_baby_bear_fri_round;
TACHYON_C_EXPORT tachyon_mi355x_baby_bear_duplex_challenger* tachyon_mi355x_baby_bear_duplex_challenger_create(
    int external_matrix, unsigned rate);
TACHYON_C_EXPORT tachyon_mi355x_baby_bear_duplex_challenger* tachyon_mi355x_baby_bear_duplex_challenger_clone(
    const tachyon_mi355x_baby_bear_duplex_challenger* c);
TACHYON_C_EXPORT void tachyon_mi355x_baby_bear_duplex_challenger_destroy(
    tachyon_mi355x_baby_bear_duplex_challenger* c);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_duplex_challenger_observe(tachyon_mi355x_baby_bear_duplex_challenger* c,
                                                                        const uint32_t* values, size_t count);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_duplex_challenger_sample(tachyon_mi355x_baby_bear_duplex_challenger* c,
                                                                       uint32_t* out, size_t count);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_duplex_challenger_sample_ext(
    tachyon_mi355x_baby_bear_duplex_challenger* c, void* out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_duplex_challenger_sample_bits(
    tachyon_mi355x_baby_bear_duplex_challenger* c, unsigned bits, uint32_t* out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_duplex_challenger_check_witness(
    tachyon_mi355x_baby_bear_duplex_challenger* c, unsigned bits, uint32_t witness);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_duplex_challenger_state(
    const tachyon_mi355x_baby_bear_duplex_challenger* c, uint32_t* out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_duplex_challenger_grind(tachyon_mi355x_baby_bear_duplex_challenger* c,
                                                                      unsigned bits, uint32_t* witness_out,
                                                                      void* stream);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_duplex_challenger_grind_range(
    tachyon_mi355x_baby_bear_duplex_challenger* c, unsigned bits, uint64_t from, uint64_t to, uint32_t* witness_out,
    void* stream);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_merkle_tree_open_batch(tachyon_mi355x_baby_bear_merkle_tree* tree,
                                                                     const size_t* indices, size_t count,
                                                                     void* const* rows_out, void* siblings_out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_opening_answer_queries(tachyon_mi355x_baby_bear_fri_opening* h,
                                                                         const size_t* indices, size_t count,
                                                                         void* sibling_values_out,
                                                                         void* siblings_out);
TACHYON_C_EXPORT tachyon_mi355x_baby_bear_fri_proof* tachyon_mi355x_baby_bear_fri_opening_prove(
    tachyon_mi355x_baby_bear_fri_opening* h, tachyon_mi355x_baby_bear_duplex_challenger* challenger,
    const tachyon_mi355x_baby_bear_fri_round* rounds, size_t num_rounds, size_t num_queries,
    unsigned proof_of_work_bits);
TACHYON_C_EXPORT void tachyon_mi355x_baby_bear_fri_proof_destroy(tachyon_mi355x_baby_bear_fri_proof* proof);
TACHYON_C_EXPORT size_t tachyon_mi355x_baby_bear_fri_proof_num_commits(const tachyon_mi355x_baby_bear_fri_proof* proof);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_proof_commits(const tachyon_mi355x_baby_bear_fri_proof* proof,
                                                                void* out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_proof_final_eval(const tachyon_mi355x_baby_bear_fri_proof* proof,
                                                                   void* out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_proof_pow_witness(const tachyon_mi355x_baby_bear_fri_proof* proof,
                                                                    uint32_t* out);
TACHYON_C_EXPORT size_t tachyon_mi355x_baby_bear_fri_proof_num_queries(const tachyon_mi355x_baby_bear_fri_proof* proof);
TACHYON_C_EXPORT size_t tachyon_mi355x_baby_bear_fri_proof_query_index(const tachyon_mi355x_baby_bear_fri_proof* proof,
                                                                       size_t q);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_proof_query_steps(const tachyon_mi355x_baby_bear_fri_proof* proof,
                                                                    size_t q, void* sibling_values_out,
                                                                    void* siblings_out);
TACHYON_C_EXPORT int tachyon_mi355x_baby_bear_fri_proof_query_input(const tachyon_mi355x_baby_bear_fri_proof* proof,
                                                                    size_t q, size_t round, void* const* rows_out,
                                                                    void* siblings_out);

/* ---- communicators and library-level sharded entry points ------------------
 * One process per MI355X: a multi-process C/C++ caller (benchmark/msm/
 * msm_benchmark_gpu.cc:57-69 or vendors/circom/prover_main.cc:116-128 under a
 * launcher) hands the library a communicator and the library does the
 * exchange itself.  Backends:
 *   rccl -- RCCL over xGMI: _comm_init_rccl (ncclCommInitRank on the current
 *     device from a 128-byte ncclUniqueId that rank 0 got from
 *     _comm_unique_id and shared) or _comm_from_rccl (wrap the caller's
 *     ncclComm_t, not owned).  All-gathers are ncclAllGather, the NTT
 *     all-to-all one ncclGroupStart/End of ncclSend/ncclRecv pairs on the
 *     plan's stream.
 *   host -- the HOST-STAGED FALLBACK (_comm_create_host): two callbacks
 *     exchange host buffers (all_gather: every rank's `bytes` in rank order;
 *     all_to_all: world blocks of `bytes`, block h to / from rank h); device
 *     data are staged through the host.  For ranks RCCL refuses (two ranks on
 *     one GPU: "Duplicate GPU detected") and CPU rehearsal backends (gloo). */
typedef struct tachyon_mi355x_comm tachyon_mi355x_comm;
typedef int (*tachyon_mi355x_all_gather_fn)(void* user, const void* send, void* recv, size_t bytes);
typedef int (*tachyon_mi355x_all_to_all_fn)(void* user, const void* send, void* recv, size_t bytes);
/* writes the 128-byte ncclUniqueId to out (cap >= 128); returns its size or 0 */
TACHYON_C_EXPORT int tachyon_mi355x_comm_unique_id(void* out, size_t cap);
TACHYON_C_EXPORT tachyon_mi355x_comm* tachyon_mi355x_comm_init_rccl(const void* unique_id, int world, int rank);
TACHYON_C_EXPORT tachyon_mi355x_comm* tachyon_mi355x_comm_from_rccl(void* nccl_comm);
TACHYON_C_EXPORT tachyon_mi355x_comm* tachyon_mi355x_comm_create_host(int world, int rank,
                                                                     tachyon_mi355x_all_gather_fn all_gather,
                                                                     tachyon_mi355x_all_to_all_fn all_to_all,
                                                                     void* user);
TACHYON_C_EXPORT void tachyon_mi355x_comm_destroy(tachyon_mi355x_comm* comm);
/* every rank's `bytes` of host memory, gathered in rank order into recv
 * (world x bytes): the exchange the sharded entries use, for callers that
 * combine their own partial results */
TACHYON_C_EXPORT void tachyon_mi355x_comm_all_gather(tachyon_mi355x_comm* comm, const void* send, void* recv,
                                                    size_t bytes);
TACHYON_C_EXPORT int tachyon_mi355x_comm_world(const tachyon_mi355x_comm* comm);
TACHYON_C_EXPORT int tachyon_mi355x_comm_rank(const tachyon_mi355x_comm* comm);
TACHYON_C_EXPORT const char* tachyon_mi355x_comm_backend(const tachyon_mi355x_comm* comm);
/* The four-step NTT of this rank's slab: stage 1, the all-to-all over `comm`,
 * stage 2 (layouts as _ntt4_stage; plan world/rank must be comm's).  Ordered
 * on the plan's stream; d_out is ready there (the host backend returns with
 * the exchange done and stage 2 enqueued). */
TACHYON_C_EXPORT void tachyon_mi355x_bn254_ntt4_run(tachyon_mi355x_bn254_ntt4* plan, tachyon_mi355x_comm* comm,
                                                   int inverse, const tachyon_bn254_fr* d_in,
                                                   tachyon_bn254_fr* d_out);

/* G2 MSM contexts (Groth16's B-in-G2, BLS12-381 config 4); same semantics as
 * the G1 *_msm_gpu entry points. */
typedef struct tachyon_bn254_g2_msm_gpu* tachyon_bn254_g2_msm_gpu_ptr;
typedef struct tachyon_bls12_381_g2_msm_gpu* tachyon_bls12_381_g2_msm_gpu_ptr;
TACHYON_C_EXPORT tachyon_bn254_g2_msm_gpu_ptr tachyon_bn254_g2_create_msm_gpu(uint8_t degree);
TACHYON_C_EXPORT void tachyon_bn254_g2_destroy_msm_gpu(tachyon_bn254_g2_msm_gpu_ptr ptr);
TACHYON_C_EXPORT tachyon_bn254_g2_jacobian* tachyon_bn254_g2_affine_msm_gpu(
    tachyon_bn254_g2_msm_gpu_ptr ptr, const tachyon_bn254_g2_affine* bases, const tachyon_bn254_fr* scalars,
    size_t size);
TACHYON_C_EXPORT tachyon_bls12_381_g2_msm_gpu_ptr tachyon_bls12_381_g2_create_msm_gpu(uint8_t degree);
TACHYON_C_EXPORT void tachyon_bls12_381_g2_destroy_msm_gpu(tachyon_bls12_381_g2_msm_gpu_ptr ptr);
TACHYON_C_EXPORT tachyon_bls12_381_g2_jacobian* tachyon_bls12_381_g2_affine_msm_gpu(
    tachyon_bls12_381_g2_msm_gpu_ptr ptr, const tachyon_bls12_381_g2_affine* bases,
    const tachyon_bls12_381_fr* scalars, size_t size);

/* Curve-generic extension API.  curve: 0 bn254_g1, 1 bn254_g2, 2 bls12_381_g1,
 * 3 bls12_381_g2.  A context is any *_msm_gpu_ptr / *_msm_ptr of that curve. */
/* Affine result written to out_affine (identity = all zero bytes). */
TACHYON_C_EXPORT void tachyon_mi355x_msm_gpu_affine(int curve, void* ctx, const void* bases, const void* scalars,
                                                    size_t size, void* out_affine);
/* The windows [w_begin, w_end) of the MSM only (window bits: the context's
 * set_window_bits, else the size's default; W = ceil((bits + 1) / c)):
 * sum over them of 2^(c w) * S_w, S_w = window w's bucket sum
 * (pippenger_base.h:59-77 restricted to the range).  Ranges that tile
 * [0, W) sum to the full MSM -- the multi-GPU window split, every rank
 * holding all points.  Affine result as in _msm_gpu_affine. */
TACHYON_C_EXPORT void tachyon_mi355x_msm_gpu_window_range_affine(int curve, void* ctx, const void* bases,
                                                                 const void* scalars, size_t size,
                                                                 unsigned w_begin, unsigned w_end,
                                                                 void* out_affine);
/* `count` MSMs over the same `len` bases (device memory of the current
 * device, e.g. a KZG SRS) in one recode / sort / accumulation / reduction:
 * MSM g takes scalars[g len, (g+1) len) (host or device; zero scalars pad
 * shorter ones) and writes its affine result to out_affine[g].  Runs on the
 * context's own device even after set_devices (the bases live there).  Window
 * bits: set_window_bits if forced, else 8 up to 2^13 points per MSM and 10
 * from 2^14 (or one MSM's default where larger).  Returns 1, or 0 (nothing
 * written) when the bases are not device memory; count x len must stay below
 * 2^31 and count at most 4096 (else the call aborts with a message, as
 * every failure of this library does). */
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_batch_affine(int curve, void* ctx, const void* bases, size_t len,
                                                        const void* scalars, size_t count, void* out_affine);
/* Fixed-base folding (bases known ahead, e.g. a proving key; an extension,
 * no reference counterpart -- the result is the same MSM).  _plan_windows:
 * W for `size` points under the context's window bits.  _fold_bases: from
 * `size` device-resident affine bases, `fold` x `size` affine points into
 * out_bases (device): copy k = 2^(k c W / fold) * P_i.  _folded_affine: the
 * MSM of `size` device scalars over such a table (same size, same window
 * bits), with W / fold window sums instead of W.  Both return 1, or 0
 * (nothing written) when fold does not divide W or a pointer is not device
 * memory. */
TACHYON_C_EXPORT unsigned tachyon_mi355x_msm_gpu_plan_windows(int curve, const void* ctx, size_t size);
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_fold_bases(int curve, void* ctx, const void* bases, size_t size,
                                                      unsigned fold, void* out_bases);
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_folded_affine(int curve, void* ctx, const void* folded_bases,
                                                         const void* scalars, size_t size, unsigned fold,
                                                         void* out_affine);
/* Contexts for the C++ plugin boundary (include/tachyon_mi355x_msm.h):
 * VariableBaseMSMGpu<Point>(mem_pool, stream) (variable_base_msm_gpu.h:16-18)
 * over any of the four groups, its work on `stream` (hipStream_t; NULL = a
 * stream the context owns; the call returns with the stream synchronised).
 * _run: the MSM of bases[0..n) and scalars[0..n) (host or device pointers)
 * written as `form` -- 0 affine {x,y}; 1 projective / 2 jacobian {x,y,z},
 * identity (1,1,0); 3 xyzz {x,y,zz,zzz}, identity (1,1,0,0).  Returns 1, or
 * 0 (out untouched) when bases_size != scalars_size, as IcicleMSM::Run
 * (icicle_msm_bn254_g1.cc:30-33) and PippengerAdapter (:55-59) return false. */
TACHYON_C_EXPORT void* tachyon_mi355x_msm_gpu_create(int curve, void* stream);
TACHYON_C_EXPORT void tachyon_mi355x_msm_gpu_destroy(int curve, void* ctx);
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_run(int curve, void* ctx, const void* bases, size_t bases_size,
                                               const void* scalars, size_t scalars_size, int form, void* out);
/* _run_points: the same with bases given in `base_form` -- 0 affine {x,y}, 1
 * projective {x,y,z} (x/z, y/z), 2 jacobian {x,y,z} (x/z^2, y/z^3), 3 xyzz
 * {x,y,zz,zzz} (x/zz, y/zzz); z (zz) = 0 is the identity -- normalised to
 * affine on the device by batch inversion first: VariableBaseMSM<Point> for
 * the non-affine point types the reference instantiates
 * (variable_base_msm_unittest.cc:30-33; Bucket = the point's own add type,
 * pippenger_base.h:18-28).  Returns 1, or 0 (out untouched) on a size
 * mismatch. */
/* _sharded_affine: this rank's shard (bases / scalars of `size` points, host
 * or device; 0 allowed) over `comm`: the local partial, one all-gather of
 * every rank's partial, the group sum in rank order -- every rank writes the
 * whole MSM's affine result (the kParallelTerm split, pippenger_adapter.h:82-113,
 * across processes). */
TACHYON_C_EXPORT void tachyon_mi355x_msm_gpu_sharded_affine(int curve, void* ctx, tachyon_mi355x_comm* comm,
                                                           const void* bases, const void* scalars, size_t size,
                                                           void* out_affine);
/* The partition of an n_total-point MSM over `world` ranks that this library
 * runs fastest (measured on MI355X): point shards, or the
 * hybrid of P = world / Q point groups x Q window groups -- rank r takes
 * point group r / Q ([start, start + count) of the global input) over window
 * range r % Q ([w_begin, w_end) of the W windows at window_bits).  Point
 * shards: window_groups 1, window_bits 0 (the shard's own default), w_begin 0,
 * w_end 0 (all windows).  Returns 1, or 0 for a rank outside [0, world). */
typedef struct tachyon_mi355x_msm_shard {
  size_t start, count;
  unsigned point_groups, window_groups, window_bits, w_begin, w_end;
} tachyon_mi355x_msm_shard;
TACHYON_C_EXPORT int tachyon_mi355x_msm_shard_plan(int curve, size_t n_total, int world, int rank,
                                                  tachyon_mi355x_msm_shard* out);
/* _sharded_plan_affine: this rank's part of `plan` (its point group's
 * bases / scalars, `plan->count` points, host or device) over `comm`: the
 * windows [w_begin, w_end) at window_bits (all windows and the shard's
 * default bits for a point shard), one all-gather of every rank's partial
 * and their group sum -- every rank writes the whole MSM's affine result and
 * returns 1.  A rank whose local part fails still enters the exchange with a
 * failure flag, so no rank is left waiting in the collective: then EVERY rank
 * returns 0 (out untouched, the message on stderr) instead of aborting.
 * A plan that does not match the call fails the same way, before any local
 * work: point_groups x window_groups != the communicator's world, w_begin >
 * w_end, w_end above the window count of window_bits for the curve, a null
 * plan or an unknown curve id (the exchanged record has one size on every
 * curve, so such a rank still joins the all-gather). */
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_sharded_plan_affine(int curve, void* ctx, tachyon_mi355x_comm* comm,
                                                                const tachyon_mi355x_msm_shard* plan,
                                                                const void* bases, const void* scalars,
                                                                void* out_affine);
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_run_points(int curve, void* ctx, const void* bases, size_t bases_size,
                                                      int base_form, const void* scalars, size_t scalars_size,
                                                      int form, void* out);
TACHYON_C_EXPORT void tachyon_mi355x_msm_gpu_set_window_bits(int curve, void* ctx, unsigned c);
/* `windows` windows of two widths for the later plain runs of the context: with
 * c_lo = floor((bits + 1) / windows), the top bits + 1 - windows c_lo windows are
 * c_lo + 1 bits wide and the rest c_lo, bits + 1 in all (the signed digits of a
 * bits-bit scalar); sort keys are bucket indices.  0 = off (the size's default
 * plan).  Only a plain run takes them: a batch, a fold or forced window bits
 * are refused while they are set (those entry points return 0), and a window
 * range aborts.  Returns 1, or 0 (nothing changed) for a layout whose widths
 * leave 2 .. 26 bits or whose bucket indices need more than 24 key bits, with
 * window bits forced, and with one or two windows per sort group set
 * (_set_variant bits 2-3 = 1 or 2; 3, all windows in one group, is accepted). */
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_set_mixed_windows(int curve, void* ctx, unsigned windows);
/* The running-sum segment length of BN254 G1's window sums for the later runs
 * of the context (tests and tuning): a power of two from 2 to 256, cut to the
 * buckets of a window; 0 = the size's own.  Other curves keep the setting and
 * do not read it.  Every length computes the same MSM.  Returns 1, or 0
 * (nothing changed) for another length. */
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_set_window_segment(int curve, void* ctx, unsigned length);
/* The layout of `windows` mixed-width windows for the curve's scalar field (no
 * GPU needed): c_lo, the number of wide windows (the top ones), the sort-key
 * bits, and windows + 1 bit offsets and bucket offsets (the last = the totals).
 * Any output may be NULL.  Returns 0 where set_mixed_windows refuses. */
TACHYON_C_EXPORT int tachyon_mi355x_msm_mixed_layout(int curve, unsigned windows, unsigned* c_lo, unsigned* n_wide,
                                                     unsigned* key_bits, unsigned* bit_offsets,
                                                     unsigned* bucket_offsets);
TACHYON_C_EXPORT void tachyon_mi355x_msm_gpu_set_profile(int curve, void* ctx, int on);
/* kernel-variant bits for A/B tuning in one process (0 = default schedule).
 * Every accepted variant computes the same MSM; returns 0 (nothing changed)
 * for bits outside 0x3FFFFBF | 1 << 27 (bits 0-25 but 6; bit 27: the uniform
 * window plan where mixed widths are the size's default; bit 23: two-level window sums
 * for the G2 / BLS12-381 G1 / FIPS reductions, measured slower; bit 24: the
 * G2 window segment sums in two passes; bit 25: the limb-field G1
 * accumulations read their entries by 8-byte loads, not LDS-staged chunks).
 * Also 0 (nothing changed) for bits 2-3 = 1 or 2 (one or two windows per sort
 * group) while _set_mixed_windows is in force: the next run would abort. */
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_set_variant(int curve, void* ctx, int variant);
/* device ms of the last run with profiling on: h2d, recode, sort, prep (bounds +
 * chunk scan), acc (the bucket-accumulation kernel alone), reduce, total,
 * accumulation launches (8 floats; of the last point chunk when the run was divided) */
TACHYON_C_EXPORT void tachyon_mi355x_msm_gpu_last_timings(int curve, const void* ctx, float* out8);
/* Point chunks the last run was split into: > 1 when the working set did not
 * fit the free device memory (DetermineMsmDivisionsForMemory,
 * icicle_msm_utils.cc:10-68; TACHYON_MSM_MEM_LIMIT caps the free bytes) or when
 * host-resident inputs were uploaded chunk by chunk under the kernels. */
TACHYON_C_EXPORT size_t tachyon_mi355x_msm_gpu_last_divisions(int curve, const void* ctx);
/* Memory planning, read-only.  _run_bytes: the estimate (with its 10 % margin)
 * of the device working set of a `size`-point run under the context's window
 * bits and variant -- what the division into point chunks and the fold-table
 * fit are decided from; with batch_count > 0 the estimate for a batch of
 * batch_count MSMs of `size` points each (_batch_affine).  _held_bytes: the
 * bytes of the working buffers the context holds now (grown by its runs, kept
 * for the next).  With set_devices active both report the lead shard, as
 * _last_schedule does.  0 for a null context. */
TACHYON_C_EXPORT size_t tachyon_mi355x_msm_gpu_run_bytes(int curve, const void* ctx, size_t size, size_t batch_count);
TACHYON_C_EXPORT size_t tachyon_mi355x_msm_gpu_held_bytes(int curve, const void* ctx);
/* Schedule of the last run (of its last point chunk): bit 0 the recode fused
 * with the first radix pass, bit 1 onesweep passes fed by the recode's digit
 * counts, bit 2 7-byte LDS staging in the recode scatter, bit 3 an
 * accumulation over the 29-bit-limb field (BN254 G1; BN254 G2's lane pair),
 * bit 4 the lane-pair G2 accumulation, bit 5 over the 28-bit-limb field
 * (BLS12-381 G1 / G2), bit 6 the chain-flag debug check ran, bit 7 the
 * limb-field accumulation read its sorted entries through LDS (64-byte chunks
 * by LDS-DMA; BN254 / BLS12-381 G1, BLS12-381 G2), bit 8 windows of two
 * widths (set_mixed_windows, or the default of BN254 G1 from 2^26 points). */
TACHYON_C_EXPORT unsigned tachyon_mi355x_msm_gpu_last_schedule(int curve, const void* ctx);
/* Diagnostic: mixed additions per second (G/s) of the curve's bucket
 * accumulation field code in registers on the current device (no gathers, no
 * bucket runs; ~0.1 s): the VALU ceiling the bench prices the accumulation
 * against.  field_bits: BN254 G1 29 (its 29-bit-limb field) or 32 (FIPS);
 * BLS12-381 G1 28 (14 x 28-bit limbs); BN254 G2 29 / BLS12-381 G2 28 (the
 * lane-pair Fq2 of the G2 accumulation, whole G2 additions, two lanes each);
 * returns 0 for other widths. */
TACHYON_C_EXPORT double tachyon_mi355x_msm_madd_ceiling(int curve, int field_bits);
/* One process, several MI355X: every later MSM of this context splits its
 * points into `count` contiguous shards, shard k on device device_ids[k]
 * (its own host thread and stream; host inputs are uploaded per shard over
 * that device's link, device inputs owned by another device are copied
 * peer-to-peer), and adds the shard results on the host -- the reference's
 * kParallelTerm chunk-and-sum (pippenger_adapter.h:82-113) and its GPU
 * divisions loop (icicle_msm_bn254_g1.cc:50-73), across devices.  The
 * reference pins device 0 (msm_gpu.h:54-56); with this, benchmark/msm and the
 * scroll_halo2 bridge reach every GPU without torch.  Ids may repeat (several
 * shards on one GPU).  count <= 1 returns to the context's own device.
 * Returns 1, or 0 (nothing changed) for an id outside [0, device count).
 * Environment: TACHYON_MSM_GPU_DEVICES="0,1,2,3" applies it to every new
 * context (the C-ABI create functions included). */
TACHYON_C_EXPORT int tachyon_mi355x_msm_gpu_set_devices(int curve, void* ctx, const int* device_ids, size_t count);
/* The shards of the last multi-device run: for each (up to cap) its wall ms
 * (upload or peer copy + MSM), point count and device; returns the number of
 * shards (0 for a single-device context).  Any output pointer may be NULL. */
TACHYON_C_EXPORT size_t tachyon_mi355x_msm_gpu_last_shards(int curve, const void* ctx, float* shard_ms,
                                                           size_t* shard_points, int* shard_devices, size_t cap);
/* window bits / windows the planner picks for a plain run of `size` points
 * (mixed widths: the narrow windows' bits) */
TACHYON_C_EXPORT void tachyon_mi355x_msm_plan(int curve, size_t size, unsigned* c, unsigned* windows);
/* Host-side group arithmetic on affine points (multi-GPU partial sums):
 * out = sum of `count` affine points. */
TACHYON_C_EXPORT void tachyon_mi355x_affine_sum(int curve, const void* points, size_t count, void* out_affine);
/* Jacobian -> affine. */
TACHYON_C_EXPORT void tachyon_mi355x_jacobian_to_affine(int curve, const void* jacobian, void* out_affine);

/* Synthetic inputs generated on the device (bench / tests):
 *   scalars: splitmix64 counter stream, BigInt::Random halving, Montgomery
 *   bases:   chunks of `chunk` points, chunk j = k_j * G, 2 k_j * G, 4 k_j * G ...
 * field: 1 bn254_fr, 3 bls12_381_fr.  d_out is device memory. stream may be NULL. */
TACHYON_C_EXPORT void tachyon_mi355x_gen_scalars(int field, uint64_t seed, size_t start, size_t n, void* d_out,
                                                 void* stream);
TACHYON_C_EXPORT void tachyon_mi355x_gen_bases(int curve, uint64_t seed, size_t n, size_t chunk, void* d_out,
                                               void* stream);
/* points [start, start + n) of that same sequence (any start; the chunk that
 * holds `start` is advanced by doublings): a rank's shard of the global input, so N ranks compute the N = 1 MSM. */
TACHYON_C_EXPORT void tachyon_mi355x_gen_bases_at(int curve, uint64_t seed, size_t start, size_t n, size_t chunk,
                                                  void* d_out, void* stream);

/* Elementwise device parity kernels (prime_field_correctness_gpu_test.cc,
 * (non_)affine_point_correctness_gpu_test.cc).  field: 0 bn254_fq, 1 bn254_fr,
 * 2 bls12_381_fq, 3 bls12_381_fr; op: 0 add 1 sub 2 mul 3 sqr 4 neg 5 inv
 * 6 to_mont 7 from_mont 8 dbl 9 a times the plain constant b (the NTT's
 * twiddle product: Shoup on BN254 Fr/Fq, a any 256-bit value) 10 a b - b a
 * and 11 a b - a^2 through the fused one-reduction a b - c d of the XYZZ
 * y coordinates.  Host buffers in, host buffer out. */
TACHYON_C_EXPORT void tachyon_mi355x_field_op(int field, int op, const void* a, const void* b, void* out,
                                              size_t count);
/* point op: 0 add (affine + affine), 1 double, 2 add-mixed into xyzz of a. Affine in/out. */
TACHYON_C_EXPORT void tachyon_mi355x_ec_op(int curve, int op, const void* a, const void* b, void* out, size_t count);

/* Elementwise device parity kernels of the carry-free limb fields of the hot
 * kernels, on RAW limbs (no conversion in or out: the caller sets every limb).
 * family: 0 f29 (BN254 Fq, N = 9 limbs of 29 bits, 8 words), 1 f28 (BLS12-381
 * Fq, N = 14 limbs of 28 bits, 12 words), 2 fr29 (BN254 Fr, N = 9).  `in` holds
 * `count` elements of in_words and `out` of out_words 32-bit words each
 * (tachyon_mi355x_limb_op_words; 0 for an unknown op), operands in the order
 * given, N limbs each.  Families 0 and 1, one lane per element:
 *   0 mul(a,b) 1 mul_add(a,b,e) 2 mul2_add(a,b,c,d) 3 mul2_add(a,b,c,d,e)
 *   4 sqr(a) 5 sqr_add(a,e) 6 normalize(a) 7 from32(words) 8 to32(a) -> words
 *   9 is_zero_mod_p(a) -> 1 word  10 reduce_shl5 / reduce(a)
 *   11 from_shifted(x2,y2) 12 madd(acc,x2,y2) 13 add(acc,acc) 14 dbl(acc) of
 *   acc29_core / acc28_core: acc = X, Y, ZZ, ZZZ; out = acc and `special`.
 * Families 0 and 1, a lane pair per element (pair29 / pair28; every Fq2 value
 * is its c0 limbs then its c1 limbs, lane h works on component h):
 *   20 pzero(a) -> 2 words  21 from_shifted(x2,y2) 22 madd(acc,x2,y2)
 *   23 add(acc,acc) 24 dbl(acc): out = acc (4 Fq2 values), then both lanes'
 *   `special`.
 *   32 + 8 kind + k: kind 0 pmul<K>(a,b) 1 pmul_add<K>(a,b,e) 2 psqr<K>(a)
 *   3 psqr_add<K>(a,e); k: 0 kK4 1 kK8 2 kK16 3 kK32 4 kK32r3 5 kK8r1 -- only
 *   the pairs (kind, K) the point formulas instantiate.
 * Family 2: 0 mont(a,b) 1 shoup(a,w,wq) 2 reduce(a) 3 from_words(8 words)
 *   4 to_canonical_words(a) -> 8 words  5 radix4(x[4], 4 Shoup twiddles w,wq)
 *   6 radix4(x[4], 4 R'-form twiddles) 7 radix4_last(x[4], w,wq)
 *   8 radix2(x[2], w,wq) 9 radix2_last(x[2]).
 * Host buffers in and out. */
TACHYON_C_EXPORT void tachyon_mi355x_limb_op(int family, int op, const uint32_t* in, uint32_t* out, size_t count);
TACHYON_C_EXPORT int tachyon_mi355x_limb_op_words(int family, int op, int* in_words, int* out_words);

/* Groth16 prover over a circom zkey (no reference C-ABI --
 * the reference drives this path from C++: vendors/circom/prover_main.cc:82-160,
 * QuadraticArithmeticProgram::WitnessMapFromMatrices
 * (quadratic_arithmetic_program.h:24-113), CreateProofWithAssignment(NoZK)
 * (tachyon/zk/r1cs/groth16/prove.h:52-186)).  The zkey bytes (v1, BN254 or
 * BLS12-381) are parsed and the proving key uploaded once at create; a proof
 * uploads only the witness.  Field elements are Montgomery form.
 *   info: out4 = {curve (0 bn254, 1 bls12_381), num_vars, num_public, domain_size}
 *   prove: full = num_vars assignments (full[0] = 1; host or device pointer),
 *          r, s = blinding scalars or NULL for zero (the NoZK proof);
 *          out_a: G1 affine, out_b: G2 affine, out_c: G1 affine (canonical).
 *   witness_map: the h evaluations on the coset (domain_size Fr) to host memory.
 *   last_timings (profiling on): upload, qap, msm_a, msm_b2, msm_b1, msm_l,
 *          msm_h, total -- ms, 8 floats (msm_l: the witness and h MSMs, run as
 *          one MSM over C1 | H1 since the proof only uses their sum; msm_h 0).
 * Multi-GPU split of prove (one process per GPU):
 *   prove_partials: this rank's shard (contiguous ceil(count / world) chunk
 *          `rank` of every MSM's points, the kParallelTerm split of
 *          pippenger_adapter.h:82-113) of the proof's MSMs, after the full
 *          witness map; writes partials_size() bytes (an opaque blob of
 *          XYZZ sums, identical layout on every rank of one build).
 *          with_b1 != 0 runs the B-in-G1 MSM (required when r != 0).
 *   assemble: `world` blobs (one per rank, any order, concatenated -- the
 *          result of one all-gather) -> the proof, as prove() would return.
 *   prove(full, r, s) == assemble(prove_partials(full, r != 0, 0, 1), 1, r, s). */
typedef struct tachyon_mi355x_groth16_prover tachyon_mi355x_groth16_prover;
TACHYON_C_EXPORT tachyon_mi355x_groth16_prover* tachyon_mi355x_groth16_prover_create(const uint8_t* zkey,
                                                                                     size_t len);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_prover_destroy(tachyon_mi355x_groth16_prover* prover);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_prover_info(const tachyon_mi355x_groth16_prover* prover,
                                                         uint32_t* out4);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_prove(tachyon_mi355x_groth16_prover* prover, const void* full,
                                                   size_t count, const void* r, const void* s, void* out_a,
                                                   void* out_b, void* out_c);
/* One-process multi-device proofs (no reference counterpart; the reference's
 * prover_main.cc:116-128 runs one process on one GPU): every later
 * tachyon_mi355x_groth16_prove runs the multi-rank split on these devices --
 * one host thread per entry runs the witness map and its 1/count chunk of
 * every MSM (_prove_partials with rank = entry, world = count), and the
 * partials are added on the host (_assemble); the proof equals the
 * single-device one.  Ids may repeat (provers sharing a GPU on separate
 * streams); count <= 1 returns to the single-device prover.  Returns 0 and
 * changes nothing when an id is out of range. */
TACHYON_C_EXPORT int tachyon_mi355x_groth16_set_devices(tachyon_mi355x_groth16_prover* prover, const int* device_ids,
                                                        size_t count);
TACHYON_C_EXPORT size_t tachyon_mi355x_groth16_partials_size(const tachyon_mi355x_groth16_prover* prover);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_prove_partials(tachyon_mi355x_groth16_prover* prover, const void* full,
                                                            size_t count, int with_b1, uint32_t rank,
                                                            uint32_t world, void* out);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_assemble(tachyon_mi355x_groth16_prover* prover, const void* parts,
                                                      size_t world, const void* r, const void* s, void* out_a,
                                                      void* out_b, void* out_c);
/* The proof across the ranks of `comm` (one process per GPU): every rank runs
 * the witness map and its chunk of every MSM (_prove_partials with the
 * comm's rank / world), one all-gather of the partials blobs, and the same
 * assembly -- every rank writes the same proof, equal to the single-GPU one. */
TACHYON_C_EXPORT void tachyon_mi355x_groth16_prove_sharded(tachyon_mi355x_groth16_prover* prover,
                                                          tachyon_mi355x_comm* comm, const void* full, size_t count,
                                                          const void* r, const void* s, void* out_a, void* out_b,
                                                          void* out_c);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_witness_map(tachyon_mi355x_groth16_prover* prover, const void* full,
                                                         size_t count, void* out_h);
/* Proving-key setup (no reference counterpart: the reference keeps no
 * per-key device state): builds the fixed-base fold tables the proofs of
 * shard (rank, world) use -- B in G2, the grouped A + witness/h G1 MSM (one
 * device) or A / B1 / witness+h (shards) -- each at the largest fold up to
 * the variant's that fits the device next to the MSM's working set
 * (TACHYON_MSM_MEM_LIMIT caps the free bytes, as for the MSM); no table
 * (fold 1) runs plain MSMs, and a grouped MSM that does not fit runs as
 * separate MSMs.  Proofs without it prepare themselves on first use.  After
 * set_devices it prepares every device's prover for its entry of the split.
 * Returns the table bytes held (summed over devices); _prover_folds writes
 * the folds chosen by the last prepare: B2, grouped G1 (0 = separate MSMs),
 * A, B1 (0 = not built), witness + h (0 = grouped). */
TACHYON_C_EXPORT size_t tachyon_mi355x_groth16_prepare(tachyon_mi355x_groth16_prover* prover, uint32_t rank,
                                                       uint32_t world, int with_b1);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_prover_folds(const tachyon_mi355x_groth16_prover* prover,
                                                          uint32_t* out5);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_set_profile(tachyon_mi355x_groth16_prover* prover, int on);
/* A/B: variant bit 0 runs A and the witness + h MSM as two MSMs (round 4);
 * clear (default) as one grouped MSM over their own bases (one recode / sort
 * / accumulation / reduction; single-device proofs).  Bits 1-3 pick the fold
 * of the G2 B query (a table of its points times 2^(k c W / F), built on the
 * first proof; _msm_gpu_fold_bases), bits 4-6 the fold of the grouped G1
 * MSM's bases: 0 the default (B2 16 copies, G1 4), k = 1..5 2^(k-1) copies (1 =
 * none), each lowered to the largest power of two dividing the MSM's window
 * count.  Same proof for every variant; returns 0 for other values. */
TACHYON_C_EXPORT int tachyon_mi355x_groth16_set_variant(tachyon_mi355x_groth16_prover* prover, int variant);
/* Window bits of the proof's MSMs (0 = each MSM's size default): A (and B in
 * G1), the merged witness + h MSM, B in G2.  Tuning / A/B; the proof is the
 * same for every choice. */
TACHYON_C_EXPORT void tachyon_mi355x_groth16_set_msm_window_bits(tachyon_mi355x_groth16_prover* prover, unsigned c_a,
                                                               unsigned c_lh, unsigned c_b2);
TACHYON_C_EXPORT void tachyon_mi355x_groth16_last_timings(const tachyon_mi355x_groth16_prover* prover,
                                                          float* out8);
/* zkey curve (0 bn254, 1 bls12_381) without building a prover. */
TACHYON_C_EXPORT int tachyon_mi355x_zkey_curve(const uint8_t* zkey, size_t len);
/* wtns v2 -> Montgomery field elements of the curve's scalar field
 * (wtns.h:99-117).  Writes min(count, cap) elements to out (may be NULL);
 * returns the witness count. */
TACHYON_C_EXPORT size_t tachyon_mi355x_wtns_parse(int curve, const uint8_t* wtns, size_t len, void* out,
                                                  size_t cap);

/* KZG commitments with a device-resident SRS (the reference's
 * tachyon/crypto/commitments/kzg/kzg.h is C++ only).  curve: 0 bn254_g1,
 * 2 bls12_381_g1.  Field elements Montgomery form, points affine.
 *   unsafe_setup: size a power of two; SRS = [tau^i] G and [L_i(tau)] G over
 *     the size-n domain (UnsafeSetup :173-207), built and kept on the device;
 *   downsize: returns 0 if n >= N (Downsize :210-215);
 *   get_srs: the N points (lagrange = 0 powers of tau, 1 Lagrange) to host;
 *   commit: MSM of the first len SRS points with `scalars` (host or device
 *     pointer) -- Commit (lagrange = 0) / CommitLagrange (1), :217-258.
 *     Returns 1, or 0 with out_affine untouched when len > N (the reference
 *     returns false: DoMSM trims the bases to min(N, len), then the MSM
 *     refuses bases/scalars of different sizes, :267-290). */
typedef struct tachyon_mi355x_kzg tachyon_mi355x_kzg;
TACHYON_C_EXPORT tachyon_mi355x_kzg* tachyon_mi355x_kzg_create(int curve);
TACHYON_C_EXPORT void tachyon_mi355x_kzg_destroy(tachyon_mi355x_kzg* kzg);
TACHYON_C_EXPORT void tachyon_mi355x_kzg_unsafe_setup(tachyon_mi355x_kzg* kzg, size_t size, const void* tau);
TACHYON_C_EXPORT size_t tachyon_mi355x_kzg_n(const tachyon_mi355x_kzg* kzg);
TACHYON_C_EXPORT int tachyon_mi355x_kzg_downsize(tachyon_mi355x_kzg* kzg, size_t n);
TACHYON_C_EXPORT void tachyon_mi355x_kzg_get_srs(const tachyon_mi355x_kzg* kzg, int lagrange, void* out);
TACHYON_C_EXPORT int tachyon_mi355x_kzg_commit(tachyon_mi355x_kzg* kzg, int lagrange, const void* scalars,
                                               size_t len, void* out_affine);
/* Batch commitments (ResizeBatchCommitments / Commit(v, state, index) /
 * GetBatchCommitments, kzg.h:116-165,296-307): `count` polynomials,
 * scalars[i] of lens[i] elements (host or device), their commitments written
 * affine to out_affine[i], normalised together with one field inversion
 * (BatchNormalize).  Polynomials of similar length run as batched MSMs
 * (groups closed when zero-padding would more than double their work or at
 * the batched MSM's size limits), the rest as single MSMs: any count and any
 * mix of lengths <= N is accepted.  Returns 1, or 0 (nothing written) when
 * any lens[i] > N. */
TACHYON_C_EXPORT int tachyon_mi355x_kzg_commit_batch(tachyon_mi355x_kzg* kzg, int lagrange,
                                                     const void* const* scalars, const size_t* lens, size_t count,
                                                     void* out_affine);

/* KZG openings: the family's CreateOpeningProof (kzg/gwc.h:83-122,
 * kzg/shplonk.h:84-226, grouping in commitments/polynomial_openings.h) on
 * polynomials that stay in device memory.  Polynomials are coefficient
 * vectors of any length >= 0, lowest degree first, host or device, ragged
 * within a call; an opening is (poly_idx[i], points[i], values[i]), points
 * and values host arrays of 32-byte Montgomery elements.  A polynomial's
 * identity is its index.
 *
 * The transcript is the caller's (a TranscriptWriter behind the callbacks):
 *   squeeze_challenge(ctx, out_fr)  writes the challenge, Montgomery form;
 *   write_to_proof(ctx, affine)     returns 0 when the write failed.
 * They are called in the reference's order -- scheme 0 (GWC): v, then every
 * W_g in group order; scheme 1 (SHPlonk): y, v, write H, u, write Q.
 *
 * create_opening_proof also copies the commitments it wrote to
 * out_affine[0 .. *out_count).  Returns 0 with no device work and no callback
 * made when: an index is out of range, a polynomial is longer than N, an
 * array is null with a nonzero count, two SHPlonk openings of one
 * (polynomial, point) claim different values, cap is below the number of
 * commitments (groups for GWC, 2 for SHPlonk), SHPlonk is given no opening
 * at all (GWC then writes nothing and returns 1).  Returns 0 after the fact when
 * a write_to_proof returned 0 or SHPlonk's Z_{T \ 0}(u) is zero (the reference
 * CHECKs); it never aborts for these.
 *
 * evaluate_batch: out[i] = polys[poly_idx[i]](points[i]), the empty
 * polynomial evaluating to 0 (one launch per level for the whole batch).
 * last_open_timings: milliseconds (stream events) of the last call's phases:
 * evaluate, combine, divide, commit. */
typedef struct {
  void (*squeeze_challenge)(void* ctx, void* out_fr);
  int (*write_to_proof)(void* ctx, const void* affine_commitment);
  void* ctx;
} tachyon_mi355x_kzg_transcript;
TACHYON_C_EXPORT int tachyon_mi355x_kzg_evaluate_batch(tachyon_mi355x_kzg* kzg, const void* const* polys,
                                                       const size_t* lens, size_t num_polys, const size_t* poly_idx,
                                                       const void* points, size_t count, void* out);
TACHYON_C_EXPORT int tachyon_mi355x_kzg_create_opening_proof(tachyon_mi355x_kzg* kzg, int scheme,
                                                             const void* const* polys, const size_t* lens,
                                                             size_t num_polys, const size_t* poly_idx,
                                                             const void* points, const void* values,
                                                             size_t num_openings,
                                                             const tachyon_mi355x_kzg_transcript* transcript,
                                                             void* out_affine, size_t cap, size_t* out_count);
TACHYON_C_EXPORT void tachyon_mi355x_kzg_last_open_timings(const tachyon_mi355x_kzg* kzg, float* out_ms);
/* The polynomial kernels on their own (curve: 0 bn254, 2 bls12-381 scalar
 * field; no SRS).  Inputs and outputs host or device.
 *   linear_combination: out[k] = sum_i coeffs[i] polys[i][k] - d [k == 0] for
 *     k < out_len, which must equal the longest input; d may be null (0).
 *   divide_by_roots: poly / prod_j (X - roots[j]), remainders dropped: the
 *     quotient's max(len, nroots) - nroots coefficients to out_quotient;
 *     out_remainders (or null) receives, per root, the remainder of its step
 *     (the value at roots[j] of the quotient by the roots before it).
 * Return 0 on a null array with a nonzero count or a wrong out_len. */
TACHYON_C_EXPORT int tachyon_mi355x_kzg_poly_linear_combination(int curve, const void* const* polys,
                                                                const size_t* lens, const void* coeffs, size_t count,
                                                                const void* d, void* out, size_t out_len);
TACHYON_C_EXPORT int tachyon_mi355x_kzg_poly_divide_by_roots(int curve, const void* poly, size_t len,
                                                             const void* roots, size_t nroots, void* out_quotient,
                                                             void* out_remainders);
/* The grouping and validation alone: host code, no GPU needed.  out receives
 * 64-bit words: the group count, then per group the point count, the points
 * (4 words each, as given), the polynomial count and the polynomial indices;
 * *out_words their number.  A group's points are in the field's order.
 * Returns 0 on the refusals above (n: the SRS size the lengths are checked
 * against) or when cap words do not suffice (*out_words is still set). */
TACHYON_C_EXPORT int tachyon_mi355x_kzg_opening_plan(int curve, int scheme, const size_t* lens, size_t num_polys,
                                                     size_t n, const size_t* poly_idx, const void* points,
                                                     const void* values, size_t num_openings, uint64_t* out,
                                                     size_t cap, size_t* out_words);

/* PLONK grand products: the polynomial Z of the Halo2 permutation, lookup and
 * shuffle arguments (zk/plonk/permutation/grand_product_argument.h:17-122 and
 * its callers permutation_prover_impl.h:24-86, lookup/halo2/prover_impl.h:
 * 126-138, shuffle/prover_impl.h:77) on columns that stay in device memory.
 *
 * A factor is f(j) = values[j] + m t(j) + c over the rows j < n, with t by
 * kind: 0 none (the term is dropped), 1 the column `table`, 2 the label
 * delta^label omega^j of permutation column `label`, computed on the device.
 * A poly job is a numerator and a denominator factor list: ratio(j) = prod
 * num(j) / prod den(j), and 0 where the denominator is 0 (the batch inverse's
 * rule, math/base/groups.h:124-180).  A chain is chain_lens[c] consecutive
 * jobs of `polys`: z[0] = 1 in its first job and the previous job's
 * z[usable_rows] in every next one; z[j+1] = z[j] ratio(j) for j <
 * usable_rows; rows usable_rows+1 .. n-1 receive that job's blinds in order
 * (zk/base/blinder.h:33-45).  All chains of a call run as one set of four
 * launches.
 *
 * Elements are 32-byte Montgomery values, canonical on output.  Columns and
 * out_z[i] (n elements per job) are host or device memory; blinds (per job
 * n - usable_rows - 1 elements, job after job), omega, delta and out_last
 * (num_chains elements: every chain's final z[usable_rows], or null) are host
 * memory.  Inputs are never written.
 *
 * Returns 1, or 0 with nothing written and no GPU call made when: field is
 * not 0 (bn254 Fr) or 2 (bls12-381 Fr); n == 0, usable_rows >= n or
 * n >= 2^31; an array is null with a nonzero count (blinds only when
 * n - usable_rows - 1 > 0, omega and delta only with a kind-2 factor); a kind
 * is above 2; a kind-1 factor has no table; a job has no factor at all; an
 * output overlaps an input column or another output; the call has more than
 * 2^30 tiles (jobs x ceil(n / tile_rows)).  A HIP failure returns 0 with a
 * message on stderr; the call never aborts.
 *
 * tile_rows: the rows one workgroup owns; walk_tiles: the tile products one
 * step of the carry walk takes.  last_timings: milliseconds (stream events)
 * of the last call's passes: ratios, carries, apply. */
typedef struct {
  const void* values;
  const void* table;
  uint32_t kind;
  uint32_t label;
  uint8_t m[32], c[32];
} tachyon_mi355x_gp_factor;
typedef struct {
  const tachyon_mi355x_gp_factor* num;
  size_t num_count;
  const tachyon_mi355x_gp_factor* den;
  size_t den_count;
} tachyon_mi355x_gp_poly;
TACHYON_C_EXPORT int tachyon_mi355x_grand_product_chains(int field, size_t n, size_t usable_rows, const void* omega,
                                                         const void* delta, const tachyon_mi355x_gp_poly* polys,
                                                         const size_t* chain_lens, size_t num_chains,
                                                         const void* blinds, void* const* out_z, void* out_last);
TACHYON_C_EXPORT size_t tachyon_mi355x_grand_product_tile_rows(void);
TACHYON_C_EXPORT size_t tachyon_mi355x_grand_product_walk_tiles(void);
TACHYON_C_EXPORT void tachyon_mi355x_grand_product_last_timings(float* out_ms);

/* Log-derivative lookup: the multiplicities m(X) and the grand sum phi(X) of
 * zk/lookup/log_derivative_halo2/prover_impl.h:99-155 (ComputeMPoly,
 * ComputeMPolys) and :186-316 (ComputeLogDerivatives, CreateGrandSumPoly,
 * CreateGrandSumPolys) on columns that stay in device memory.  beta is drawn
 * after the m polynomials are committed, hence two calls.
 *
 * A lookup has num_inputs >= 1 compressed input columns f_0 .. f_{K-1} and
 * one compressed table column t; u = usable_rows of n rows; `count` runs over
 * all lookups of all circuits, which the caller flattens.
 *
 * m_polys: the entries (i, t[i] as a canonical integer) for i < u are sorted
 * by the integer alone, ties by ascending i (base::StableSort).  For every
 * input column and row j < u the canonical value of f_k[j] is searched with
 * BinarySearchByKey (base/containers/container_util.h:169-185): left = 0,
 * right = u, mid = left + (right - left) / 2, and the FIRST equal hit
 * returns.  A hit adds 1 to the counter of that entry's original row; a miss
 * adds nothing and is no error.  With duplicate table values the row that
 * receives the count is the one this bisection lands on.  out_m[l][i] = the
 * counter for i < u and 0 for u <= i < n (m is not blinded); out_misses[l]
 * (or null) = the input values of lookup l found nowhere in t[0..u).
 *
 * grand_sums: L[i] = sum_k 1 / (f_k[i] + beta) - m[i] / (t[i] + beta) for
 * i < u, where a zero denominator contributes 0 (the batch inverse skips
 * zeros, math/base/groups.h:124-143).  out_phi[l][0] = 0, out_phi[l][i] =
 * sum_{j<i} L[j] for i < u, out_phi[l][u] = 0, and the rows u+1 .. n-1 receive
 * that lookup's blinds in order (zk/base/blinder.h:33-45).  out_totals (or
 * null): per lookup the sum of L over all u rows, which is 0 for a lookup
 * that balances and is not part of the polynomial.
 *
 * Elements are 32-byte Montgomery values, canonical on output.  Columns, m,
 * blinds (per lookup n - usable_rows - 1 elements, lookup after lookup),
 * out_m[l], out_phi[l] (n elements each) and out_totals are host or device
 * memory; beta, the descriptor arrays and out_misses are host memory.  Inputs
 * are never written.
 *
 * Both return 1, or 0 with nothing written and no GPU call made when: field
 * is not 0 (bn254 Fr) or 2 (bls12-381 Fr); n is no power of two, n < 2 or
 * n > 2^30; usable_rows == 0 or usable_rows >= n; a lookup has no inputs; an
 * array or a column is null with a nonzero count (blinds only when
 * n - usable_rows - 1 > 0), or beta is null; an output overlaps an input, a
 * table, an m or another output.  The blinds are taken to hold exactly
 * n - usable_rows - 1 elements per phi: capi/log_lookup_validate.h refuses
 * any other count for a caller that knows the array's length, as the Python
 * binding does.  A HIP failure, more than 2^32 - 1 (input, row) pairs in one
 * lookup or more than 2^30 workgroups in one launch return 0 with a message
 * on stderr; the calls never abort.
 *
 * tile_rows: the rows one workgroup of the grand sum owns (the carry scan
 * takes 256 tile sums per step).  work_bytes: the device memory the larger of
 * the two calls holds for `count` lookups of at most max_inputs inputs with
 * every column staged from the host (0 on a failure; needs a device).
 * last_timings: 5 values, milliseconds (stream events) of the last calls'
 * phases: sort, count (m_polys), sums A, B, C (grand_sums). */
typedef struct {
  const void* const* inputs;
  size_t num_inputs;
  const void* table;
} tachyon_mi355x_log_lookup;
TACHYON_C_EXPORT int tachyon_mi355x_log_lookup_m_polys(int field, size_t n, size_t usable_rows,
                                                       const tachyon_mi355x_log_lookup* lookups, size_t count,
                                                       void* const* out_m, uint64_t* out_misses);
TACHYON_C_EXPORT int tachyon_mi355x_log_lookup_grand_sums(int field, size_t n, size_t usable_rows, const void* beta,
                                                          const tachyon_mi355x_log_lookup* lookups,
                                                          const void* const* m, size_t count, const void* blinds,
                                                          void* const* out_phi, void* out_totals);
TACHYON_C_EXPORT size_t tachyon_mi355x_log_lookup_tile_rows(void);
TACHYON_C_EXPORT size_t tachyon_mi355x_log_lookup_work_bytes(size_t n, size_t max_inputs, size_t count);
TACHYON_C_EXPORT void tachyon_mi355x_log_lookup_last_timings(float* out_ms);

/* Halo2 lookup: the permuted columns A' and S' of zk/lookup/halo2/
 * permute_expression_pair.h:29-142 (PermuteExpressionPair, called from
 * lookup/halo2/prover_impl.h:74-95) on columns that stay in device memory: the
 * step between the compressed pair and tachyon_mi355x_lookup_grand_product.
 *
 * A pair is one lookup's compressed input column A and compressed table
 * column S, n elements each, u = usable_rows of them used; `count` runs over
 * all lookups of all circuits, which the caller flattens.  "Value order" is
 * the order of the canonical integers (ToBigInt()), not of the Montgomery
 * limbs.
 *
 *   A'[0..u) is A[0..u) in ascending value order.  Row i < u is a first row
 *   when i = 0 or A'[i] != A'[i-1], else a repeated row; R = the number of
 *   repeated rows, r(i) the rank of repeated row i among them by ascending i.
 *   leftover[0..R) is the multiset S[0..u) less one instance of each distinct
 *   value of A', in ascending value order.  S'[i] = A'[i] on a first row and
 *   leftover[R - 1 - r(i)] on a repeated row (the reference hands the
 *   leftover out in ascending order, each to the last repeated row not yet
 *   served).  Rows u .. n-1 of A' and then of S' are the caller's blinds:
 *   per pair n - u values for A' followed by n - u for S' (Blind with
 *   include_last_row, zk/base/blinder.h:33-45), pair after pair.
 *
 * Outputs are the bytes of the elements they came from (Montgomery form, not
 * reduced again).  out_misses[l] (or null) = the distinct values of A[0..u)
 * of pair l found nowhere in S[0..u); the reference aborts on one.  Here a
 * pair with misses has unspecified rows < u in its two outputs (its blind
 * rows are still written, nothing is read or written out of bounds) and every
 * other pair of the call is exact.
 *
 * Columns, blinds, out_input[l] and out_table[l] (n elements each) are host
 * or device memory; the descriptor and pointer arrays and out_misses are host
 * memory.  Inputs are never written.
 *
 * permute_pairs returns 1 when it ran, with or without misses, and 0 with
 * nothing written and no GPU call made when: field is not 0 (bn254 Fr) or 2
 * (bls12-381 Fr); n is no power of two, n < 2 or n > 2^30; usable_rows == 0
 * or usable_rows >= n; an array, a column, an output or blinds is null with a
 * nonzero count; an output overlaps another output or any column of the call.
 * count == 0 returns 1 and makes no GPU call.  The blinds are taken to hold
 * exactly 2 (n - usable_rows) elements per pair: capi/
 * lookup_permute_validate.h refuses any other count for a caller that knows
 * the array's length, as the Python binding does.  A HIP failure or more than
 * 2^30 workgroups in one launch return 0 with a message on stderr; the call
 * never aborts.
 *
 * work_bytes: the device memory one call holds for `count` pairs of n rows
 * with every column and output in host memory (0 on a failure; needs a
 * device).  last_timings: 4 values, milliseconds (stream events) of the last
 * call's phases: sort, search, ranks, write. */
typedef struct {
  const void* input;
  const void* table;
} tachyon_mi355x_lookup_pair;
TACHYON_C_EXPORT int tachyon_mi355x_lookup_permute_pairs(int field, size_t n, size_t usable_rows,
                                                         const tachyon_mi355x_lookup_pair* pairs, size_t count,
                                                         const void* blinds, void* const* out_input,
                                                         void* const* out_table, uint64_t* out_misses);
TACHYON_C_EXPORT size_t tachyon_mi355x_lookup_permute_work_bytes(size_t n, size_t count);
TACHYON_C_EXPORT void tachyon_mi355x_lookup_permute_last_timings(float* out_ms);

/* PLONK quotient: the vanishing argument's h(X) (zk/plonk/vanishing/
 * circuit_polynomial_builder.h:199-245, the Scroll shape; vanishing_utils.h:
 * 65-112, 167-196; vanishing_prover_impl.h:106-112) on device-resident
 * polynomials.
 *
 * A graph is a flattened expression (graph_evaluator.h, calculation.h,
 * value_source.h), serialised field by field.  A source's `kind` follows
 * value_source.h: 0 Constant, 1 Intermediate, 2 Fixed, 3 Advice, 4 Instance,
 * 5 Challenge, 6 Beta, 7 Gamma, 8 Theta, 9 Y, 10 PreviousValue; `index` is
 * the constant, intermediate, column or challenge index and `rotation_index`
 * (column kinds only) an index into the graph's `rotations`.  A calculation's
 * `op` follows calculation.h: 0 Add, 1 Sub, 2 Mul (a, b), 3 Square, 4 Double,
 * 5 Negate, 7 Store (a), 6 Horner: a is the initial value, b the factor and
 * the parts are parts[parts_begin .. parts_begin + parts_count) of the graph:
 * v = a; for each part: v = v b + part.  The result goes to intermediate
 * `target`.  A graph's value on a row is its last calculation's target, and
 * zero for a graph with no calculation.  A column read at rotation r is
 * col[(row + r) mod n] (zk/base/rotation.h:45-51, scale 1).
 *
 * A term group is what one evaluator adds to the per-row accumulator of one
 * circuit, in the reference's order:
 *   0 gates        acc = graph(PreviousValue = acc)   (custom_gate_evaluator.h)
 *   1 permutation  permutation_evaluator.h:25-108 over num_z = ceil(m /
 *                  (cs_degree - 2)) products, m = num_perm_columns; nothing
 *                  for m = 0
 *   2 lookup       lookup/halo2/evaluator.h:66-128 with graph = the compressed
 *                  (A + beta)(S + gamma) of the argument (PreviousValue = 0)
 *   3 shuffle      shuffle/evaluator.h:71-119 with graph = the input's A +
 *                  gamma and graph2 = the shuffle's S + gamma
 * each term folded as acc = acc y + term.
 *
 * tachyon_mi355x_quotient_evaluate_part runs one group over caller-held
 * evaluations on one size-n coset: every column (table columns, l_first,
 * l_last, l_active_row, z, a_perm, s_perm, sigmas) is n evaluations, host or
 * device, and acc (n elements, host or device) is read and written in place.
 * For the permutation x_scale is delta_start times the coset's extended omega
 * power (beta zeta w_ext^i) and omega the size-n generator: the label of
 * column k on row j is x_scale omega^j delta^k.
 *
 * tachyon_mi355x_quotient_h_poly is the driver: every polynomial is given by
 * its n coefficients (host or device).  With P = 2^(extended_k - k) parts
 * (extended_k: the least e with 2^e >= n (cs_degree - 1)) it evaluates, for
 * each part i, everything on the coset zeta w_ext^i <w> with one batched
 * transform, runs the groups of every circuit in order (gates, permutation,
 * lookups, shuffles; the accumulator carries from circuit to circuit),
 * multiplies by 1 / (zeta^n w_ext^(n i) - 1) while it scatters the part to
 * ext[j P + i], and after the last part transforms back from the coset
 * zeta <w_ext>.  out (host or device) receives n (cs_degree - 1)
 * coefficients, or all n P with full != 0.  w_ext is ext_gen (the extended
 * domain's generator, of order exactly 2^extended_k; else the call returns 0
 * with a message), or with ext_gen null the field's 2^extended_k root of the
 * active generator set; the size-n generator is w_ext^P.
 * Fixed-column and sigma cosets are recomputed for every part.
 *
 * Elements are 32-byte Montgomery values, canonical on output.  Constants,
 * challenges, theta, beta, gamma, y, zeta, delta, ext_gen, omega and x_scale
 * are host memory.  Inputs are never written.
 *
 * Both return 1, or 0 with nothing written and no GPU call made when: field
 * is not 0 (bn254 Fr) or 2 (bls12-381 Fr); a needed pointer is null; n is not
 * a power of two, n < 2 or n > 2^30; cs_degree < 3; extended_k exceeds the
 * field's two-adicity (or 30); a kind or op is out of range; a constant,
 * column, rotation, challenge or Horner-part index is out of range; a target
 * is >= num_intermediates; an intermediate is read before the calculation
 * that writes it; a permutation column is not of kind 2, 3 or 4 or names no
 * column; num_z differs from ceil(m / (cs_degree - 2)); a group kind is above
 * 3.  h_poly also returns 0, with a message and nothing written, for an
 * ext_gen of another order and for a zeta with zeta^n w_ext^(n i) = 1 on some
 * part (X^n - 1 has no inverse there).  A HIP failure or a failed allocation
 * returns 0 with a message on stderr; the calls never abort.
 *
 * work_bytes: the device memory one h_poly call of this shape holds at its
 * peak (one part's cosets, the extended buffer, the accumulator, the spill
 * workspace, the program upload and the transform tables), before anything
 * is allocated; 0 for a shape the call refuses.  held_bytes: what the last
 * h_poly call did hold.  tile_rows: the rows one workgroup owns; fast_slots:
 * the intermediates of a lowered program that live in LDS (more spill to a
 * [slot][row] workspace).  last_timings: milliseconds (stream events) of the
 * last call's transforms, gates, permutation, lookups, shuffles, scatter and
 * final inverse transform (evaluate_part fills its own group's entry). */
typedef struct {
  uint32_t kind, index, rotation_index;
} tachyon_mi355x_quotient_source;
typedef struct {
  uint32_t op;
  tachyon_mi355x_quotient_source a, b;
  uint32_t parts_begin, parts_count;
  uint32_t target;
} tachyon_mi355x_quotient_calc;
typedef struct {
  const tachyon_mi355x_quotient_calc* calcs;
  size_t num_calcs;
  const tachyon_mi355x_quotient_source* parts;
  size_t num_parts;
  const void* constants;
  size_t num_constants;
  const int32_t* rotations;
  size_t num_rotations;
  size_t num_intermediates;
} tachyon_mi355x_quotient_graph;
/* one circuit's columns and challenges (the evaluation table of a graph) */
typedef struct {
  const void* const* fixed;
  size_t num_fixed;
  const void* const* advice;
  size_t num_advice;
  const void* const* instance;
  size_t num_instance;
  const void* challenges;
  size_t num_challenges;
} tachyon_mi355x_quotient_table;
typedef struct {
  int field;
  size_t n;
  uint32_t cs_degree;
  int32_t last_row; /* the permutation's -(blinding_factors + 1) rotation */
  const void *theta, *beta, *gamma, *y;
  const void *l_first, *l_last, *l_active_row;
} tachyon_mi355x_quotient_params;
typedef struct {
  uint32_t kind;
  const tachyon_mi355x_quotient_graph* graph;
  const tachyon_mi355x_quotient_graph* graph2;
  const void* const* z;
  size_t num_z;
  const void *a_perm, *s_perm;
  const tachyon_mi355x_quotient_source* perm_columns;
  size_t num_perm_columns;
  const void* const* sigmas;
  const void *x_scale, *omega, *delta;
} tachyon_mi355x_quotient_group;
/* what the circuits of one proof share */
typedef struct {
  const tachyon_mi355x_quotient_graph* gates; /* null: no gate group */
  const tachyon_mi355x_quotient_source* perm_columns;
  size_t num_perm_columns;
  const void* const* sigmas;
  const tachyon_mi355x_quotient_graph* lookups;
  size_t num_lookups;
  const tachyon_mi355x_quotient_graph* shuffles; /* 2 per shuffle: input, shuffle */
  size_t num_shuffles;
} tachyon_mi355x_quotient_system;
typedef struct {
  tachyon_mi355x_quotient_table table;
  const void* const* perm_z;
  size_t num_perm_z;
  const void* const* lookup_z; /* num_lookups each */
  const void* const* lookup_a_perm;
  const void* const* lookup_s_perm;
  const void* const* shuffle_z; /* num_shuffles */
} tachyon_mi355x_quotient_circuit;
TACHYON_C_EXPORT int tachyon_mi355x_quotient_evaluate_part(const tachyon_mi355x_quotient_params* params,
                                                           const tachyon_mi355x_quotient_table* table,
                                                           const tachyon_mi355x_quotient_group* group, void* acc);
TACHYON_C_EXPORT int tachyon_mi355x_quotient_h_poly(const tachyon_mi355x_quotient_params* params,
                                                    const tachyon_mi355x_quotient_system* system,
                                                    const tachyon_mi355x_quotient_circuit* circuits,
                                                    size_t num_circuits, const void* zeta, const void* delta,
                                                    const void* ext_gen, int full, void* out);
TACHYON_C_EXPORT size_t tachyon_mi355x_quotient_work_bytes(const tachyon_mi355x_quotient_params* params,
                                                           const tachyon_mi355x_quotient_system* system,
                                                           const tachyon_mi355x_quotient_circuit* circuits,
                                                           size_t num_circuits);
TACHYON_C_EXPORT size_t tachyon_mi355x_quotient_held_bytes(void);
/* The lowered program of one term group, on the host alone (no GPU call; the
 * arguments of evaluate_part, acc unused): out[0] its instructions, out[1]
 * the field products among them (Mul and Square), out[2] the column elements
 * it reads per row, out[3] the slots it needs (those beyond fast_slots
 * spill).  Returns 0 for a group evaluate_part refuses. */
TACHYON_C_EXPORT int tachyon_mi355x_quotient_program_stats(const tachyon_mi355x_quotient_params* params,
                                                           const tachyon_mi355x_quotient_table* table,
                                                           const tachyon_mi355x_quotient_group* group, size_t* out);
TACHYON_C_EXPORT size_t tachyon_mi355x_quotient_tile_rows(void);
TACHYON_C_EXPORT size_t tachyon_mi355x_quotient_fast_slots(void);
TACHYON_C_EXPORT void tachyon_mi355x_quotient_last_timings(float* out_ms);

/* delete a Jacobian returned by an *_msm / *_msm_gpu entry point (for callers
 * that cannot use C++ delete, e.g. ctypes). */
TACHYON_C_EXPORT void tachyon_mi355x_jacobian_destroy(int curve, void* jacobian);
TACHYON_C_EXPORT const char* tachyon_mi355x_version(void);
TACHYON_C_EXPORT int tachyon_mi355x_device_count(void);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* TACHYON_MI355X_H_ */
