/* C++ GPU-NTT hook for Tachyon's UnivariateEvaluationDomain, header-only over
 * the C-ABI of libtachyon_mi355x.so.
 *
 * Replaces (same shape and semantics):
 *   IcicleNTTHolder<F>   tachyon/math/polynomials/univariate/icicle/icicle_ntt_holder.h:15-63
 *                        (Create(), operator->, owns the NTT object)
 *   IcicleNTT<F>::FFT / IFFT / Run
 *                        icicle_ntt.h:53-142, icicle_ntt_bn254.cc:31-116
 *                        (in place on the host vector, natural order in and out,
 *                        the coset offset given per call; CHECK-abort on failure)
 *   UnivariateEvaluationDomain::set_icicle / FFT / IFFT dispatch
 *                        univariate_evaluation_domain.h:99,141-232 (the caller
 *                        resizes the evaluations to size() first)
 *
 * A Tachyon build with this backend keeps its set_icicle call sites and swaps
 * the holder type ("set_gpu_backend"):
 *
 *   auto holder = tachyon_mi355x::NTTHolder::Create(domain->size());
 *   // FFT: evals.evaluations_ resized to size(), then
 *   holder->FFT(evals.evaluations_, offset);      // offset: bn254::Fr, 1 = no coset
 *   holder->IFFT(poly.coefficients_, offset);
 *
 * F is any type with the layout of tachyon_bn254_fr (4 x uint64 Montgomery
 * limbs): bn254::Fr itself, or tachyon_bn254_fr.  NTT / NTTHolder go through
 * the reference's BN254 C-ABI domain (its multi-device split included).
 *
 * The other scalar field the reference's icicle backend covers,
 * IcicleNTT<bls12_381::Fr> (icicle_ntt_bls12_381.cc:31-115), is
 * FieldNTT<kBls12_381Fr> / FieldNTTHolder<kBls12_381Fr> over the
 * field-generic domain (tachyon_mi355x_ntt_domain_*, bn254 Fr too):
 *
 *   auto holder = tachyon_mi355x::FieldNTTHolder<tachyon_mi355x::kBls12_381Fr>::Create(size);
 *   holder->FFT(evals, &offset);   // bls12_381::Fr, nullptr = no coset
 *
 * The holders above bind one size.  IcicleNTTHolder<F, kField> / IcicleNTT<F,
 * kField> at the end of this header are the reference's holder unchanged:
 * Create() without a size, Init(group_gen) once, FFT / IFFT(algorithm,
 * canonical coset, container) at any power-of-two size up to the generator's
 * order, bool results. */
#ifndef TACHYON_MI355X_NTT_HOLDER_H_
#define TACHYON_MI355X_NTT_HOLDER_H_

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "tachyon_mi355x.h"

namespace tachyon_mi355x {

class NTT {
 public:
  explicit NTT(size_t size) : domain_(tachyon_bn254_univariate_evaluation_domain_create(size)) {
    size_ = tachyon_mi355x_bn254_univariate_evaluation_domain_size(domain_);
  }
  NTT(const NTT&) = delete;
  NTT& operator=(const NTT&) = delete;
  ~NTT() { tachyon_bn254_univariate_evaluation_domain_destroy(domain_); }

  size_t size() const { return size_; }

  /* IcicleNTT::FFT: evaluations (size() elements, coefficients in) in place. */
  template <class F>
  bool FFT(std::vector<F>& evals, const F* coset = nullptr) {
    return Run(evals.data(), evals.size(), coset, 0);
  }
  /* IcicleNTT::IFFT: coefficients (size() elements, evaluations in) in place. */
  template <class F>
  bool IFFT(std::vector<F>& coeffs, const F* coset = nullptr) {
    return Run(coeffs.data(), coeffs.size(), coset, 1);
  }

  /* IcicleNTT::Run on a raw host pointer; size must equal size(). */
  template <class F>
  bool Run(F* inout, size_t size, const F* coset, int inverse) {
    static_assert(sizeof(F) == sizeof(tachyon_bn254_fr), "F must have the layout of tachyon_bn254_fr");
    SetCoset(coset);
    tachyon_mi355x_bn254_univariate_evaluation_domain_transform_host(
        domain_, reinterpret_cast<tachyon_bn254_fr*>(inout), size, inverse);
    return true;  // failures abort inside the library, like the reference's CHECKs
  }

  tachyon_bn254_univariate_evaluation_domain* domain() { return domain_; }

 private:
  template <class F>
  void SetCoset(const F* coset) {
    tachyon_bn254_fr want;
    if (coset) {
      std::memcpy(&want, coset, sizeof(want));
    } else {
      want = One();
    }
    if (have_coset_ && std::memcmp(&want, &coset_, sizeof(want)) == 0) return;
    tachyon_mi355x_bn254_univariate_evaluation_domain_set_offset(domain_, &want);
    coset_ = want;
    have_coset_ = true;
  }
  static tachyon_bn254_fr One() {
    /* 1 in Montgomery form = R mod r for BN254 Fr */
    tachyon_bn254_fr one = {{0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL,
                             0x0e0a77c19a07df2fULL}};
    return one;
  }

  tachyon_bn254_univariate_evaluation_domain* domain_ = nullptr;
  size_t size_ = 0;
  tachyon_bn254_fr coset_ = {};
  bool have_coset_ = false;
};

/* Field ids of tachyon_mi355x_ntt_domain_create (1 and 3) and of
 * tachyon_mi355x_icicle_ntt_create (all three). */
enum NttField : int { kBn254Fr = 1, kBls12_381Fr = 3, kBabyBear = 4 };

/* Element and canonical BigInt sizes of a field id: 4 x uint64 Montgomery
 * limbs and a 32-byte BigInt for the two Fr fields; one uint32 Montgomery word
 * and the 8-byte BigInt<1> for BabyBear. */
template <int kField>
struct NttFieldTraits {
  static constexpr size_t kElementBytes = 32;
  static constexpr size_t kBigIntBytes = 32;
};
template <>
struct NttFieldTraits<kBabyBear> {
  static constexpr size_t kElementBytes = 4;
  static constexpr size_t kBigIntBytes = 8;
};

/* IcicleNTT<F> over the field-generic domain: the same FFT / IFFT / Run as
 * NTT above for the field kField (F: 4 x uint64 Montgomery limbs). */
template <int kField>
class FieldNTT {
 public:
  explicit FieldNTT(size_t size) : domain_(tachyon_mi355x_ntt_domain_create(kField, size)) {
    size_ = tachyon_mi355x_ntt_domain_size(domain_);
  }
  FieldNTT(const FieldNTT&) = delete;
  FieldNTT& operator=(const FieldNTT&) = delete;
  ~FieldNTT() { tachyon_mi355x_ntt_domain_destroy(domain_); }

  size_t size() const { return size_; }
  template <class F>
  bool FFT(std::vector<F>& evals, const F* coset = nullptr) {
    return Run(evals.data(), evals.size(), coset, 0);
  }
  template <class F>
  bool IFFT(std::vector<F>& coeffs, const F* coset = nullptr) {
    return Run(coeffs.data(), coeffs.size(), coset, 1);
  }
  template <class F>
  bool Run(F* inout, size_t size, const F* coset, int inverse) {
    static_assert(sizeof(F) == 4 * sizeof(uint64_t), "F must be 4 x uint64 Montgomery limbs");
    uint64_t want[4] = {0, 0, 0, 0};
    if (coset) std::memcpy(want, coset, sizeof(want));
    if (!have_coset_ || std::memcmp(want, coset_, sizeof(want)) != 0) {
      /* (all-zero = no coset: the offset 0 is not a coset of the domain) */
      tachyon_mi355x_ntt_domain_set_offset(domain_, coset ? static_cast<const void*>(want) : nullptr);
      std::memcpy(coset_, want, sizeof(want));
      have_coset_ = true;
    }
    tachyon_mi355x_ntt_domain_transform_host(domain_, inout, size, inverse);
    return true;  // failures abort inside the library, like the reference's CHECKs
  }
  tachyon_mi355x_ntt_domain* domain() { return domain_; }

 private:
  tachyon_mi355x_ntt_domain* domain_ = nullptr;
  size_t size_ = 0;
  uint64_t coset_[4] = {0, 0, 0, 0};
  bool have_coset_ = false;
};

/* IcicleNTTHolder<F> for FieldNTT<kField>. */
template <int kField>
class FieldNTTHolder {
 public:
  static FieldNTTHolder Create(size_t size) { return FieldNTTHolder(std::make_unique<FieldNTT<kField>>(size)); }
  FieldNTT<kField>* operator->() { return ntt_.get(); }
  const FieldNTT<kField>* operator->() const { return ntt_.get(); }
  FieldNTT<kField>* get() { return ntt_.get(); }

 private:
  explicit FieldNTTHolder(std::unique_ptr<FieldNTT<kField>> ntt) : ntt_(std::move(ntt)) {}
  std::unique_ptr<FieldNTT<kField>> ntt_;
};

/* IcicleNTTHolder<bn254::Fr>: owns one NTT; Create() + operator->. */
class NTTHolder {
 public:
  static NTTHolder Create(size_t size) { return NTTHolder(std::make_unique<NTT>(size)); }
  NTT* operator->() { return ntt_.get(); }
  const NTT* operator->() const { return ntt_.get(); }
  NTT* get() { return ntt_.get(); }

 private:
  explicit NTTHolder(std::unique_ptr<NTT> ntt) : ntt_(std::move(ntt)) {}
  std::unique_ptr<NTT> ntt_;
};

/* ---- the drop-in holder: Create() without a size, Init(group_gen) once, then
 * FFT / IFFT of any power-of-two size the initialised domain contains, the
 * canonical coset given per call (tachyon_mi355x_icicle_ntt_*).  A Tachyon
 * build keeps the reference's lines unchanged --
 *
 *   CHECK((*icicle_)->FFT(FFTAlgorithmToIcicleNTTAlgorithm(GetAlgorithm()),
 *                         offset_big_int_, evals));
 *   icicle_ntt_holder_ = math::IcicleNTTHolder<F>::Create();
 *   CHECK(icicle_ntt_holder_->Init(extended_domain_->group_gen()));
 *
 * -- with math::IcicleNTTHolder<F> aliased to
 * tachyon_mi355x::IcicleNTTHolder<F, kField> and ::ntt to
 * tachyon_mi355x::ntt. */
namespace ntt {
/* icicle's ntt.cu.h enumerations, in its order */
enum class NTTDir { kForward, kInverse };
enum class Ordering { kNN, kNR, kRN, kRR, kNM, kMN };
enum class NttAlgorithm { Auto, Radix2, MixedRadix };
}  // namespace ntt

/* icicle_ntt.h:43-51, the reference's fields and defaults.  Supported:
 * batch_size >= 1, columns_batch false (kBabyBear: also true, the buffer is
 * then a size x batch_size row-major matrix), ordering kNN, inputs and outputs
 * both on the host or both on the device; Init refuses anything else. */
struct IcicleNTTOptions {
  bool fast_twiddles_mode = true;
  int batch_size = 1;
  bool columns_batch = false;
  ntt::Ordering ordering = ntt::Ordering::kNN;
  bool are_inputs_on_device = false;
  bool are_outputs_on_device = false;
  bool is_async = false;
};

/* IcicleNTT<F> (icicle_ntt.h:53-102) for the field kField; F has the
 * field's element size (NttFieldTraits: 4 x uint64 Montgomery limbs, or one
 * uint32 Montgomery word for kBabyBear).  BigInt (F::BigIntTy in the
 * reference) is any trivially copyable type of the field's BigInt size holding
 * the canonical little-endian value.  With kBabyBear, options.columns_batch is
 * supported and FFTBatch / CosetLDEBatch below are available
 * (IcicleNTTHolder<BabyBear, kBabyBear>). */
template <class F, int kField>
class IcicleNTT {
 public:
  IcicleNTT() : handle_(tachyon_mi355x_icicle_ntt_create(kField, nullptr)) {}
  explicit IcicleNTT(void* stream) : handle_(tachyon_mi355x_icicle_ntt_create(kField, stream)) {}
  IcicleNTT(const IcicleNTT&) = delete;
  IcicleNTT& operator=(const IcicleNTT&) = delete;
  ~IcicleNTT() { tachyon_mi355x_icicle_ntt_destroy(handle_); }

  [[nodiscard]] bool Init(const F& group_gen, const IcicleNTTOptions& options = IcicleNTTOptions()) {
    static_assert(sizeof(F) == NttFieldTraits<kField>::kElementBytes,
                  "F must have the field's element size (4 x uint64 limbs; one uint32 for kBabyBear)");
    tachyon_mi355x_icicle_ntt_options o;
    o.fast_twiddles_mode = options.fast_twiddles_mode ? 1 : 0;
    o.batch_size = options.batch_size;
    o.columns_batch = options.columns_batch ? 1 : 0;
    o.ordering = static_cast<int>(options.ordering);
    o.are_inputs_on_device = options.are_inputs_on_device ? 1 : 0;
    o.are_outputs_on_device = options.are_outputs_on_device ? 1 : 0;
    o.is_async = options.is_async ? 1 : 0;
    return handle_ && tachyon_mi355x_icicle_ntt_init(handle_, &group_gen, &o) == 1;
  }

  template <class BigInt, class Evals>
  [[nodiscard]] bool FFT(ntt::NttAlgorithm algorithm, const BigInt& coset, Evals& evals) const {
    const std::vector<F>& evaluations = evals.evaluations();
    return Run(algorithm, coset, const_cast<F*>(evaluations.data()), static_cast<int>(evaluations.size()),
               ntt::NTTDir::kForward);
  }

  template <class BigInt, class Poly>
  [[nodiscard]] bool IFFT(ntt::NttAlgorithm algorithm, const BigInt& coset, Poly& poly) const {
    const std::vector<F>& coefficients = poly.coefficients().coefficients();
    return Run(algorithm, coset, const_cast<F*>(coefficients.data()), static_cast<int>(coefficients.size()),
               ntt::NTTDir::kInverse);
  }

  /* size: elements per transform; inout holds batch_size * size of them */
  template <class BigInt>
  [[nodiscard]] bool Run(ntt::NttAlgorithm algorithm, const BigInt& coset, F* inout, int size,
                         ntt::NTTDir dir) const {
    static_assert(sizeof(BigInt) == NttFieldTraits<kField>::kBigIntBytes &&
                      std::is_trivially_copyable<BigInt>::value,
                  "BigInt must hold the field's canonical little-endian bytes (32; 8 for kBabyBear)");
    if (!handle_ || size < 0) return false;
    return tachyon_mi355x_icicle_ntt_run(handle_, static_cast<int>(algorithm), &coset, inout,
                                         static_cast<size_t>(size), dir == ntt::NTTDir::kInverse ? 1 : 0) == 1;
  }

  /* Radix2EvaluationDomain::FFTBatch (radix2_evaluation_domain.h:99-127) on a
   * raw row-major rows x cols matrix (no Eigen here): every column transformed
   * in place on the plain domain, natural order.  kBabyBear only. */
  [[nodiscard]] bool FFTBatch(F* mat, size_t rows, size_t cols) const {
    static_assert(kField == kBabyBear, "FFTBatch: kBabyBear only");
    const uint64_t one = 1;
    return handle_ && tachyon_mi355x_icicle_ntt_run_matrix(handle_, 0, &one, mat, rows, cols, 0) == 1;
  }

  /* Radix2EvaluationDomain::CosetLDEBatch (radix2_evaluation_domain.h:129-197):
   * in (rows x cols) -> out ((rows << added_bits) x cols), the low-degree
   * extension of every column on the coset shift * <w>.  shift is the field
   * element as stored (Montgomery); it is converted to the canonical value the
   * C-ABI takes here, in the header, with one Montgomery multiplication by 1
   * (x R^-1 mod p).  kBabyBear only. */
  [[nodiscard]] bool CosetLDEBatch(const F* in, size_t rows, size_t cols, size_t added_bits, const F& shift,
                                   F* out) const {
    static_assert(kField == kBabyBear, "CosetLDEBatch: kBabyBear only");
    static_assert(sizeof(F) == 4, "BabyBear: one uint32 Montgomery word");
    constexpr uint32_t kP = 0x78000001u, kNInv = 0x77ffffffu; /* p, -p^-1 mod 2^32 */
    uint32_t m;
    std::memcpy(&m, &shift, sizeof(m));
    const uint32_t q = m * kNInv;
    uint32_t c = static_cast<uint32_t>((static_cast<uint64_t>(m) + static_cast<uint64_t>(q) * kP) >> 32);
    if (c >= kP) c -= kP;
    const uint64_t canonical = c;
    return handle_ &&
           tachyon_mi355x_icicle_ntt_coset_lde_batch(handle_, in, rows, cols, added_bits, &canonical, out) == 1;
  }

  [[nodiscard]] bool Release() { return handle_ && tachyon_mi355x_icicle_ntt_release(handle_) == 1; }

  /* log2 of the initialised order, -1 before Init / after Release */
  int log_order() const { return handle_ ? tachyon_mi355x_icicle_ntt_log_order(handle_) : -1; }
  void* stream() const { return handle_ ? tachyon_mi355x_icicle_ntt_stream(handle_) : nullptr; }
  tachyon_mi355x_icicle_ntt* handle() { return handle_; }

 private:
  tachyon_mi355x_icicle_ntt* handle_ = nullptr;
};

/* IcicleNTTHolder<F> (icicle_ntt_holder.h:15-63): empty when default
 * constructed, Create() makes the IcicleNTT; move-only. */
template <class F, int kField>
class IcicleNTTHolder {
 public:
  IcicleNTTHolder() = default;
  IcicleNTTHolder(IcicleNTTHolder&&) = default;
  IcicleNTTHolder& operator=(IcicleNTTHolder&&) = default;

  const IcicleNTT<F, kField>& operator*() const { return *get(); }
  IcicleNTT<F, kField>& operator*() { return *get(); }

  const IcicleNTT<F, kField>* operator->() const { return get(); }
  IcicleNTT<F, kField>* operator->() { return get(); }

  operator bool() const { return !!icicle_; }

  const IcicleNTT<F, kField>* get() const { return icicle_.get(); }
  IcicleNTT<F, kField>* get() { return icicle_.get(); }

  static IcicleNTTHolder Create() { return IcicleNTTHolder(std::make_unique<IcicleNTT<F, kField>>()); }

  void Release() { icicle_.reset(); }

 private:
  explicit IcicleNTTHolder(std::unique_ptr<IcicleNTT<F, kField>> icicle) : icicle_(std::move(icicle)) {}

  std::unique_ptr<IcicleNTT<F, kField>> icicle_;
};

}  // namespace tachyon_mi355x

#endif  // TACHYON_MI355X_NTT_HOLDER_H_
