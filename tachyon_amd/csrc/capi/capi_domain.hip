// C-ABI of the BN254 univariate evaluation domain and its three containers
// (include/tachyon_mi355x.h).
//
// Reference entry points restated here:
//   tachyon/c/math/polynomials/univariate/bn254_univariate_evaluation_domain.cc:22-85
//   tachyon/c/math/polynomials/univariate/bn254_univariate_evaluations.cc
//   tachyon/c/math/polynomials/univariate/bn254_univariate_dense_polynomial.cc
#include "../../../include/tachyon_mi355x.h"

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../ntt/ntt.h"
#include "../util/device_ops.h"
#include "capi_guard.h"

using namespace tachyon_amd;

namespace tachyon_amd::capi_detail {
// univariate containers hold std::vector<bn254::Fr>, like the reference
using FrC = tachyon_bn254_fr;
struct Vec {
  std::vector<FrC> v;
};
struct Domain {
  std::unique_ptr<ntt::NttDomain<Bn254Fr>> impl;
  int device = 0;  // the device the domain was created on (the multi-device primary)
  // set_devices: the four-step over several devices for the plain domain
  // (declared after impl: destroyed first, while impl's stream still exists)
  std::unique_ptr<ntt::NttMultiDevice<Bn254Fr>> multi;
  ntt::NttMultiDevice<Bn254Fr>* multi_for_plain() const {
    return multi && impl->offset().is_one() ? multi.get() : nullptr;
  }
  // In place, forward or inverse, over several devices where that applies:
  // `len` host elements (zero padded to size() by the engine) or size() device ones.
  void transform_host(Bn254Fr* v, size_t len, bool inverse) const {
    if (auto* m = multi_for_plain()) inverse ? m->inverse_host(v, len, v) : m->forward_host(v, len, v);
    else inverse ? impl->inverse_host(v, len, v) : impl->forward_host(v, len, v);
  }
  void transform_device(Bn254Fr* x, bool inverse) const {
    if (auto* m = multi_for_plain()) inverse ? m->inverse_device(x, x) : m->forward_device(x, x);
    else inverse ? impl->inverse_device(x) : impl->forward_device(x);
  }
};
// UnivariateEvaluations<RationalField<bn254::Fr>>: {numerator, denominator}
// pairs; Zero() = 0 / 1 (math/base/rational_field.h:33,199-200)
struct RationalVec {
  std::vector<FrC> num, den;
};
}  // namespace tachyon_amd::capi_detail
using tachyon_amd::capi_detail::RationalVec;
using tachyon_amd::capi_detail::Domain;
using tachyon_amd::capi_detail::FrC;
using tachyon_amd::capi_detail::Vec;

struct tachyon_bn254_univariate_evaluations : Vec {};
struct tachyon_bn254_univariate_dense_polynomial : Vec {};
struct tachyon_bn254_univariate_evaluation_domain : Domain {};
struct tachyon_bn254_univariate_rational_evaluations : RationalVec {};

namespace {
// UnivariateEvaluationDomain::FFT (univariate_evaluation_domain.h:141-182):
// empty poly -> empty evals; otherwise n evaluations.  The transform runs in
// place on the vector it returns: the in-place entry points hand over the
// caller's vector (no second host allocation -- first-touch page faults of a
// fresh 512 MiB vector cost more than the transform), the copying ones copy
// the input once.
std::vector<FrC> do_fft(const Domain* d, std::vector<FrC>&& v) {
  if (v.empty()) return std::move(v);
  const size_t len = v.size(), n = d->impl->size();
  if (len < n) v.resize(n);  // zero padding
  d->transform_host(reinterpret_cast<Bn254Fr*>(v.data()), len, false);
  return std::move(v);
}
// IFFT + RemoveHighDegreeZeros (radix2_evaluation_domain.h:218-223)
std::vector<FrC> do_ifft(const Domain* d, std::vector<FrC>&& v) {
  if (v.empty()) return std::move(v);
  const size_t len = v.size(), n = d->impl->size();
  if (len < n) v.resize(n);
  d->transform_host(reinterpret_cast<Bn254Fr*>(v.data()), len, true);
  size_t keep = v.size();
  while (keep > 0) {
    const FrC& x = v[keep - 1];
    if (x.limbs[0] | x.limbs[1] | x.limbs[2] | x.limbs[3]) break;
    --keep;
  }
  v.resize(keep);
  return std::move(v);
}
}  // namespace

extern "C" {

// ---- univariate evaluation domain over BN254 Fr ----
tachyon_bn254_univariate_evaluation_domain* tachyon_bn254_univariate_evaluation_domain_create(size_t num_coeffs) {
  GUARD_BEGIN
  auto* d = new tachyon_bn254_univariate_evaluation_domain();
  d->impl.reset(new ntt::NttDomain<Bn254Fr>(num_coeffs));
  TA_HIP(hipGetDevice(&d->device));
  return d;
  GUARD_END
}
void tachyon_bn254_univariate_evaluation_domain_destroy(tachyon_bn254_univariate_evaluation_domain* domain) {
  delete domain;
}
// Domain::Zero<Evals>() = size() zeros (univariate_evaluations.h:251-255)
tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluation_domain_empty_evals(
    const tachyon_bn254_univariate_evaluation_domain* domain) {
  GUARD_BEGIN
  auto* e = new tachyon_bn254_univariate_evaluations();
  e->v.assign(domain->impl->size(), FrC{});
  return e;
  GUARD_END
}
tachyon_bn254_univariate_rational_evaluations* tachyon_bn254_univariate_evaluation_domain_empty_rational_evals(
    const tachyon_bn254_univariate_evaluation_domain* domain) {
  GUARD_BEGIN
  auto* e = new tachyon_bn254_univariate_rational_evaluations();
  const Bn254Fr one = Bn254Fr::one();
  FrC one_c;
  memcpy(&one_c, &one, sizeof(one_c));
  e->num.assign(domain->impl->size(), FrC{});
  e->den.assign(domain->impl->size(), one_c);
  return e;
  GUARD_END
}

// ---- bn254_univariate_rational_evaluations.h (reference .cc:18-88) ----
tachyon_bn254_univariate_rational_evaluations* tachyon_bn254_univariate_rational_evaluations_create(void) {
  GUARD_BEGIN return new tachyon_bn254_univariate_rational_evaluations(); GUARD_END
}
tachyon_bn254_univariate_rational_evaluations* tachyon_bn254_univariate_rational_evaluations_clone(
    const tachyon_bn254_univariate_rational_evaluations* evals) {
  GUARD_BEGIN return new tachyon_bn254_univariate_rational_evaluations(*evals); GUARD_END
}
void tachyon_bn254_univariate_rational_evaluations_destroy(tachyon_bn254_univariate_rational_evaluations* evals) {
  delete evals;
}
size_t tachyon_bn254_univariate_rational_evaluations_len(const tachyon_bn254_univariate_rational_evaluations* evals) {
  return evals->num.size();
}
// boundary checks are the caller's, as in the reference (.cc:42)
void tachyon_bn254_univariate_rational_evaluations_set_zero(tachyon_bn254_univariate_rational_evaluations* evals,
                                                            size_t i) {
  const Bn254Fr one = Bn254Fr::one();
  evals->num[i] = FrC{};
  memcpy(&evals->den[i], &one, sizeof(FrC));
}
void tachyon_bn254_univariate_rational_evaluations_set_trivial(tachyon_bn254_univariate_rational_evaluations* evals,
                                                               size_t i, const tachyon_bn254_fr* numerator) {
  const Bn254Fr one = Bn254Fr::one();
  evals->num[i] = *numerator;
  memcpy(&evals->den[i], &one, sizeof(FrC));
}
void tachyon_bn254_univariate_rational_evaluations_set_rational(tachyon_bn254_univariate_rational_evaluations* evals,
                                                                size_t i, const tachyon_bn254_fr* numerator,
                                                                const tachyon_bn254_fr* denominator) {
  evals->num[i] = *numerator;
  evals->den[i] = *denominator;
}
// RationalField::Evaluate (rational_field.h:115): numerator / denominator;
// a zero denominator fails like the reference's unwrap (abort)
void tachyon_bn254_univariate_rational_evaluations_evaluate(
    const tachyon_bn254_univariate_rational_evaluations* evals, size_t i, tachyon_bn254_fr* value) {
  GUARD_BEGIN
  Bn254Fr d;
  memcpy(&d, &evals->den[i], sizeof(d));
  if (d.is_zero()) throw std::runtime_error("RationalField::Evaluate: zero denominator");
  util::batch_evaluate_bn254_fr(&evals->num[i], &evals->den[i], value, 1);
  GUARD_END
}
tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_rational_evaluations_batch_evaluate(
    const tachyon_bn254_univariate_rational_evaluations* evals) {
  GUARD_BEGIN
  auto* out = new tachyon_bn254_univariate_evaluations();
  out->v.resize(evals->num.size());
  util::batch_evaluate_bn254_fr(evals->num.data(), evals->den.data(), out->v.data(), out->v.size());
  return out;
  GUARD_END
}
void tachyon_mi355x_bn254_univariate_rational_evaluations_resize(tachyon_bn254_univariate_rational_evaluations* evals,
                                                                 size_t len) {
  GUARD_BEGIN
  const Bn254Fr one = Bn254Fr::one();
  FrC one_c;
  memcpy(&one_c, &one, sizeof(one_c));
  evals->num.resize(len, FrC{});
  evals->den.resize(len, one_c);
  GUARD_END
}
void tachyon_mi355x_bn254_univariate_rational_evaluations_get(
    const tachyon_bn254_univariate_rational_evaluations* evals, size_t i, tachyon_bn254_fr* numerator,
    tachyon_bn254_fr* denominator) {
  *numerator = evals->num[i];
  *denominator = evals->den[i];
}

tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_evaluation_domain_empty_poly(
    const tachyon_bn254_univariate_evaluation_domain* domain) {
  GUARD_BEGIN
  auto* p = new tachyon_bn254_univariate_dense_polynomial();
  p->v.assign(domain->impl->size(), FrC{});
  return p;
  GUARD_END
}

tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluation_domain_fft(
    const tachyon_bn254_univariate_evaluation_domain* domain, const tachyon_bn254_univariate_dense_polynomial* poly) {
  GUARD_BEGIN
  auto* e = new tachyon_bn254_univariate_evaluations();
  e->v = do_fft(domain, std::vector<FrC>(poly->v));
  return e;
  GUARD_END
}
tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluation_domain_fft_inplace(
    const tachyon_bn254_univariate_evaluation_domain* domain, tachyon_bn254_univariate_dense_polynomial* poly) {
  GUARD_BEGIN
  auto* e = new tachyon_bn254_univariate_evaluations();
  std::vector<FrC> in = std::move(poly->v);  // moved-from, as FFT(DensePoly&&)
  poly->v.clear();
  e->v = do_fft(domain, std::move(in));
  return e;
  GUARD_END
}
tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_evaluation_domain_ifft(
    const tachyon_bn254_univariate_evaluation_domain* domain, const tachyon_bn254_univariate_evaluations* evals) {
  GUARD_BEGIN
  auto* p = new tachyon_bn254_univariate_dense_polynomial();
  p->v = do_ifft(domain, std::vector<FrC>(evals->v));
  return p;
  GUARD_END
}
tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_evaluation_domain_ifft_inplace(
    const tachyon_bn254_univariate_evaluation_domain* domain, tachyon_bn254_univariate_evaluations* evals) {
  GUARD_BEGIN
  auto* p = new tachyon_bn254_univariate_dense_polynomial();
  std::vector<FrC> in = std::move(evals->v);
  evals->v.clear();
  p->v = do_ifft(domain, std::move(in));
  return p;
  GUARD_END
}

tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluations_create(void) {
  return new tachyon_bn254_univariate_evaluations();
}
tachyon_bn254_univariate_evaluations* tachyon_bn254_univariate_evaluations_clone(
    const tachyon_bn254_univariate_evaluations* evals) {
  auto* e = new tachyon_bn254_univariate_evaluations();
  e->v = evals->v;
  return e;
}
void tachyon_bn254_univariate_evaluations_destroy(tachyon_bn254_univariate_evaluations* evals) { delete evals; }
size_t tachyon_bn254_univariate_evaluations_len(const tachyon_bn254_univariate_evaluations* evals) {
  return evals->v.size();
}
void tachyon_bn254_univariate_evaluations_set_value(tachyon_bn254_univariate_evaluations* evals, size_t i,
                                                    const tachyon_bn254_fr* value) {
  GUARD_BEGIN evals->v.at(i) = *value; GUARD_END  // .at() as in the reference: OOB aborts
}
tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_dense_polynomial_create(void) {
  return new tachyon_bn254_univariate_dense_polynomial();
}
tachyon_bn254_univariate_dense_polynomial* tachyon_bn254_univariate_dense_polynomial_clone(
    const tachyon_bn254_univariate_dense_polynomial* poly) {
  auto* p = new tachyon_bn254_univariate_dense_polynomial();
  p->v = poly->v;
  return p;
}
void tachyon_bn254_univariate_dense_polynomial_destroy(tachyon_bn254_univariate_dense_polynomial* poly) {
  delete poly;
}

void tachyon_mi355x_bn254_univariate_evaluations_get_value(const tachyon_bn254_univariate_evaluations* evals,
                                                           size_t i, tachyon_bn254_fr* value) {
  GUARD_BEGIN *value = evals->v.at(i); GUARD_END
}
tachyon_bn254_fr* tachyon_mi355x_bn254_univariate_evaluations_data(tachyon_bn254_univariate_evaluations* evals) {
  return evals->v.data();
}
void tachyon_mi355x_bn254_univariate_evaluations_resize(tachyon_bn254_univariate_evaluations* evals, size_t len) {
  GUARD_BEGIN evals->v.resize(len, FrC{}); GUARD_END
}
size_t tachyon_mi355x_bn254_univariate_dense_polynomial_len(const tachyon_bn254_univariate_dense_polynomial* poly) {
  return poly->v.size();
}
void tachyon_mi355x_bn254_univariate_dense_polynomial_resize(tachyon_bn254_univariate_dense_polynomial* poly,
                                                             size_t len) {
  GUARD_BEGIN poly->v.resize(len, FrC{}); GUARD_END
}
void tachyon_mi355x_bn254_univariate_dense_polynomial_set_value(tachyon_bn254_univariate_dense_polynomial* poly,
                                                                size_t i, const tachyon_bn254_fr* value) {
  GUARD_BEGIN poly->v.at(i) = *value; GUARD_END
}
void tachyon_mi355x_bn254_univariate_dense_polynomial_get_value(
    const tachyon_bn254_univariate_dense_polynomial* poly, size_t i, tachyon_bn254_fr* value) {
  GUARD_BEGIN *value = poly->v.at(i); GUARD_END
}
tachyon_bn254_fr* tachyon_mi355x_bn254_univariate_dense_polynomial_data(tachyon_bn254_univariate_dense_polynomial* poly) {
  return poly->v.data();
}

void tachyon_mi355x_bn254_halo2_override_subgroup_generator(void) { ntt::set_bn254_fr_halo2_generator(true); }
void tachyon_mi355x_bn254_halo2_restore_subgroup_generator(void) { ntt::set_bn254_fr_halo2_generator(false); }
int tachyon_mi355x_bn254_halo2_subgroup_generator_active(void) { return ntt::bn254_fr_halo2_generator() ? 1 : 0; }

size_t tachyon_mi355x_bn254_univariate_evaluation_domain_size(const tachyon_bn254_univariate_evaluation_domain* d) {
  return d->impl->size();
}
void tachyon_mi355x_bn254_univariate_evaluation_domain_group_gen(const tachyon_bn254_univariate_evaluation_domain* d,
                                                                 tachyon_bn254_fr* out) {
  memcpy(out, &d->impl->group_gen(), sizeof(*out));
}
void tachyon_mi355x_bn254_univariate_evaluation_domain_set_offset(tachyon_bn254_univariate_evaluation_domain* d,
                                                                  const tachyon_bn254_fr* offset) {
  GUARD_BEGIN
  Bn254Fr h;
  memcpy(&h, offset, sizeof(h));
  d->impl->set_offset(h);
  GUARD_END
}
void tachyon_mi355x_bn254_univariate_evaluation_domain_transform_device(tachyon_bn254_univariate_evaluation_domain* d,
                                                                        tachyon_bn254_fr* d_data, int inverse) {
  GUARD_BEGIN d->transform_device(reinterpret_cast<Bn254Fr*>(d_data), inverse != 0); GUARD_END
}
void tachyon_mi355x_bn254_univariate_evaluation_domain_transform_host(tachyon_bn254_univariate_evaluation_domain* d,
                                                                      tachyon_bn254_fr* inout, size_t len,
                                                                      int inverse) {
  GUARD_BEGIN
  if (len != d->impl->size())
    throw std::runtime_error("transform_host: the vector must hold exactly size() elements (" + std::to_string(len) +
                             " != " + std::to_string(d->impl->size()) + ")");
  d->transform_host(reinterpret_cast<Bn254Fr*>(inout), len, inverse != 0);
  GUARD_END
}
void tachyon_mi355x_bn254_univariate_evaluation_domain_transform_batch_device(
    tachyon_bn254_univariate_evaluation_domain* d, tachyon_bn254_fr* d_data, size_t batch, int inverse) {
  GUARD_BEGIN
  if (inverse) d->impl->inverse_device(reinterpret_cast<Bn254Fr*>(d_data), batch);
  else d->impl->forward_device(reinterpret_cast<Bn254Fr*>(d_data), batch);
  GUARD_END
}
void* tachyon_mi355x_bn254_univariate_evaluation_domain_stream(tachyon_bn254_univariate_evaluation_domain* d) {
  return d->impl->stream();
}
void tachyon_mi355x_bn254_univariate_evaluation_domain_set_profile(tachyon_bn254_univariate_evaluation_domain* d,
                                                                   int on) {
  d->impl->set_profile(on != 0);
}
int tachyon_mi355x_bn254_univariate_evaluation_domain_set_variant(tachyon_bn254_univariate_evaluation_domain* d,
                                                                  int variant) {
  GUARD_BEGIN return d->impl->set_variant(variant) ? 1 : 0; GUARD_END
  return 0;
}
int tachyon_mi355x_bn254_univariate_evaluation_domain_set_devices(tachyon_bn254_univariate_evaluation_domain* d,
                                                                   const int* ids, size_t count) {
  GUARD_BEGIN
  if (count <= 1) {
    d->multi.reset();
    return 1;
  }
  const size_t n = d->impl->size();
  if (n < 4) return 0;
  int avail = 0;
  TA_HIP(hipGetDeviceCount(&avail));
  for (size_t i = 0; i < count; ++i)
    if (ids[i] < 0 || ids[i] >= avail) return 0;
  // the four-step splits R and C by a power of two: the first 2^k of the ids,
  // 2^k <= count and <= R = 2^floor(log n / 2) (devices() reports them)
  size_t use = 1;
  while (use * 2 <= count && use * 2 <= (size_t(1) << (d->impl->log_size() / 2))) use *= 2;
  if (use < 2) return 0;
  if (use == 2) {  // two parts: the one-link all-to-all costs more than the transform (see the header)
    d->multi.reset();
    return 1;
  }
  const std::vector<int> dev(ids, ids + use);
  std::unique_ptr<ntt::NttMultiDevice<Bn254Fr>> m;
  try {
    m = std::make_unique<ntt::NttMultiDevice<Bn254Fr>>(d->impl->log_size(), dev, d->device, d->impl->stream());
  } catch (const std::exception&) {  // not a power of two, too many for the size, or a bad id
    return 0;
  }
  if (!(m->root() == d->impl->group_gen())) return 0;  // another generator set was active at create
  d->multi = std::move(m);
  return 1;
  GUARD_END
  return 0;
}
size_t tachyon_mi355x_bn254_univariate_evaluation_domain_devices(const tachyon_bn254_univariate_evaluation_domain* d,
                                                                 int* ids, size_t cap) {
  if (!d->multi) return 0;
  const auto& v = d->multi->device_ids();
  for (size_t i = 0; i < v.size() && i < cap; ++i) ids[i] = v[i];
  return v.size();
}
int tachyon_mi355x_bn254_univariate_evaluation_domain_last_timings(const tachyon_bn254_univariate_evaluation_domain* d,
                                                                   float* total_ms, float* pass_ms, int max_passes) {
  const auto& t = d->impl->timings();
  if (total_ms) *total_ms = t.total;
  int np = (int)t.passes.size();
  for (int i = 0; i < np && i < max_passes; ++i) pass_ms[i] = t.passes[i];
  return np;
}

}  // extern "C"
