// C-ABI of the KZG commitment scheme (include/tachyon_mi355x.h, "KZG").
// Reference: tachyon/crypto/commitments/kzg/kzg.h (UnsafeSetup :173-207,
// Downsize :210-215, Commit/CommitLagrange :217-258, device SRS :90-114);
// errors abort like the reference's CHECKs.
#include "../../../include/tachyon_mi355x.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../kzg/kzg.h"
#include "capi_guard.h"
#include "kzg_open_validate.h"

using namespace tachyon_amd;

struct tachyon_mi355x_kzg {
  int curve;  // 0 bn254_g1, 2 bls12_381_g1
  std::unique_ptr<kzg::Kzg<Bn254G1>> bn;
  std::unique_ptr<kzg::Kzg<Bls381G1>> bls;
};

#define KZG_DISPATCH(p, ...)          \
  do {                                \
    if ((p)->curve == 0) {            \
      auto* impl = (p)->bn.get();     \
      __VA_ARGS__;                    \
    } else {                          \
      auto* impl = (p)->bls.get();    \
      __VA_ARGS__;                    \
    }                                 \
  } while (0)

extern "C" {

tachyon_mi355x_kzg* tachyon_mi355x_kzg_create(int curve) {
  GUARD_BEGIN
  if (curve != 0 && curve != 2) throw std::runtime_error("KZG curve must be 0 (bn254_g1) or 2 (bls12_381_g1)");
  auto* p = new tachyon_mi355x_kzg();
  p->curve = curve;
  if (curve == 0) p->bn = std::make_unique<kzg::Kzg<Bn254G1>>();
  else p->bls = std::make_unique<kzg::Kzg<Bls381G1>>();
  return p;
  GUARD_END
}

void tachyon_mi355x_kzg_destroy(tachyon_mi355x_kzg* p) { delete p; }

void tachyon_mi355x_kzg_unsafe_setup(tachyon_mi355x_kzg* p, size_t size, const void* tau) {
  GUARD_BEGIN
  KZG_DISPATCH(p, impl->unsafe_setup(size, *static_cast<const typename std::remove_pointer_t<decltype(impl)>::Fr*>(tau)));
  GUARD_END
}

size_t tachyon_mi355x_kzg_n(const tachyon_mi355x_kzg* p) {
  GUARD_BEGIN KZG_DISPATCH(p, return impl->n()); GUARD_END
}

int tachyon_mi355x_kzg_downsize(tachyon_mi355x_kzg* p, size_t n) {
  GUARD_BEGIN KZG_DISPATCH(p, return impl->downsize(n) ? 1 : 0); GUARD_END
}

void tachyon_mi355x_kzg_get_srs(const tachyon_mi355x_kzg* p, int lagrange, void* out) {
  GUARD_BEGIN
  KZG_DISPATCH(p, impl->copy_srs(lagrange != 0, static_cast<typename std::remove_pointer_t<decltype(impl)>::Aff*>(out)));
  GUARD_END
}

int tachyon_mi355x_kzg_commit(tachyon_mi355x_kzg* p, int lagrange, const void* scalars, size_t len,
                              void* out_affine) {
  GUARD_BEGIN
  KZG_DISPATCH(p, {
    using K = std::remove_pointer_t<decltype(impl)>;
    typename K::Aff a;
    if (!impl->commit(static_cast<const typename K::Fr*>(scalars), len, lagrange != 0, &a)) return 0;
    memcpy(out_affine, &a, sizeof(a));
    return 1;
  });
  GUARD_END
}

int tachyon_mi355x_kzg_commit_batch(tachyon_mi355x_kzg* p, int lagrange, const void* const* scalars,
                                    const size_t* lens, size_t count, void* out_affine) {
  GUARD_BEGIN
  KZG_DISPATCH(p, {
    using K = std::remove_pointer_t<decltype(impl)>;
    return impl->commit_batch(reinterpret_cast<const typename K::Fr* const*>(scalars), lens, count, lagrange != 0,
                              static_cast<typename K::Aff*>(out_affine))
               ? 1
               : 0;
  });
  GUARD_END
}

}  // extern "C"

// Openings: evaluate, GWC / SHPlonk CreateOpeningProof, the polynomial
// primitives on their own, and the grouping alone (host code).
namespace {

template <class Fr>
int linear_combination(const void* const* polys, const size_t* lens, const void* coeffs, size_t count, const void* d,
                       void* out, size_t out_len) {
  if (count != 0 && (!polys || !lens || !coeffs)) return 0;
  size_t longest = 0;
  for (size_t i = 0; i < count; ++i) {
    if (lens[i] != 0 && !polys[i]) return 0;
    longest = std::max(longest, lens[i]);
  }
  if (out_len != longest || (out_len != 0 && !out)) return 0;
  if (!out_len) return 1;
  require_gpu();
  OwnedStream stream;
  kzg::PolyOps<Fr> ops(stream.s);
  DeviceBuffer result;
  std::vector<const Fr*> dev;
  ops.stage(reinterpret_cast<const Fr* const*>(polys), lens, count, &dev);
  std::vector<typename kzg::PolyOps<Fr>::Term> terms(count);
  bool in_place = usable_in_place(out);
  for (size_t i = 0; i < count; ++i) {
    terms[i] = {dev[i], lens[i], static_cast<const Fr*>(coeffs)[i]};
    if (static_cast<const void*>(dev[i]) == out) in_place = false;
  }
  Fr* dst = in_place ? static_cast<Fr*>(out) : static_cast<Fr*>(result.ensure(out_len * sizeof(Fr)));
  ops.linear_combination(terms.data(), count, d ? *static_cast<const Fr*>(d) : Fr::zero(), dst, out_len);
  if (!in_place) TA_HIP(hipMemcpyAsync(out, dst, out_len * sizeof(Fr), hipMemcpyDefault, stream.s));
  ops.synchronize();
  return 1;
}

template <class Fr>
int divide_by_roots(const void* poly, size_t len, const void* roots, size_t nroots, void* out_quotient,
                    void* out_remainders) {
  const size_t qlen = len - std::min(len, nroots);
  if ((len != 0 && !poly) || (nroots != 0 && !roots) || (qlen != 0 && !out_quotient)) return 0;
  if (!nroots) {  // nothing to divide by: the polynomial itself
    require_gpu();
    if (len) TA_HIP(hipMemcpy(out_quotient, poly, len * sizeof(Fr), hipMemcpyDefault));
    return 1;
  }
  require_gpu();
  OwnedStream stream;
  kzg::PolyOps<Fr> ops(stream.s);
  DeviceBuffer result, rems;
  std::vector<const Fr*> dev;
  const Fr* src = static_cast<const Fr*>(poly);
  ops.stage(&src, &len, 1, &dev);
  const bool in_place = usable_in_place(out_quotient) && out_quotient != dev[0];
  Fr* dst = in_place ? static_cast<Fr*>(out_quotient) : static_cast<Fr*>(result.ensure(std::max<size_t>(1, qlen) * sizeof(Fr)));
  Fr* d_rems = static_cast<Fr*>(rems.ensure(nroots * sizeof(Fr)));
  ops.divide_by_roots(dev[0], len, static_cast<const Fr*>(roots), nroots, dst, d_rems);
  if (!in_place && qlen) TA_HIP(hipMemcpyAsync(out_quotient, dst, qlen * sizeof(Fr), hipMemcpyDefault, stream.s));
  if (out_remainders)
    TA_HIP(hipMemcpyAsync(out_remainders, d_rems, nroots * sizeof(Fr), hipMemcpyDefault, stream.s));
  ops.synchronize();
  return 1;
}

template <class Fr>
int opening_plan(int scheme, const size_t* lens, size_t num_polys, size_t n, const size_t* poly_idx, const void* points,
                 const void* values, size_t num_openings, uint64_t* out, size_t cap, size_t* out_words) {
  kzg_open::Openings o;
  o.poly = poly_idx;
  o.points = static_cast<const unsigned char*>(points);
  o.values = static_cast<const unsigned char*>(values);
  o.elem_bytes = sizeof(Fr);
  o.count = num_openings;
  kzg_open::Plan plan;
  if (!out_words || !kzg_open::make_plan(scheme, o, lens, num_polys, n, kzg::element_less<Fr>, &plan)) return 0;
  *out_words = kzg_open::flat_words(plan, sizeof(Fr));
  if (*out_words > cap || !out) return 0;
  kzg_open::flatten(plan, o, out);
  return 1;
}

}  // namespace

#define FR_DISPATCH(curve, ...)                 \
  do {                                          \
    if ((curve) == 0) {                         \
      using Fr = Bn254Fr;                       \
      __VA_ARGS__;                              \
    } else if ((curve) == 2) {                  \
      using Fr = Bls381Fr;                      \
      __VA_ARGS__;                              \
    } else {                                    \
      return 0;                                 \
    }                                           \
  } while (0)

extern "C" {

int tachyon_mi355x_kzg_evaluate_batch(tachyon_mi355x_kzg* p, const void* const* polys, const size_t* lens,
                                      size_t num_polys, const size_t* poly_idx, const void* points, size_t count,
                                      void* out) {
  GUARD_BEGIN
  KZG_DISPATCH(p, {
    using K = std::remove_pointer_t<decltype(impl)>;
    return impl->evaluate_batch(reinterpret_cast<const typename K::Fr* const*>(polys), lens, num_polys, poly_idx,
                                static_cast<const typename K::Fr*>(points), count, static_cast<typename K::Fr*>(out))
               ? 1
               : 0;
  });
  GUARD_END
}

int tachyon_mi355x_kzg_create_opening_proof(tachyon_mi355x_kzg* p, int scheme, const void* const* polys,
                                            const size_t* lens, size_t num_polys, const size_t* poly_idx,
                                            const void* points, const void* values, size_t num_openings,
                                            const tachyon_mi355x_kzg_transcript* transcript, void* out_affine,
                                            size_t cap, size_t* out_count) {
  GUARD_BEGIN
  if (!transcript) return 0;
  KZG_DISPATCH(p, {
    using K = std::remove_pointer_t<decltype(impl)>;
    const typename K::Transcript t{transcript->squeeze_challenge, transcript->write_to_proof, transcript->ctx};
    return impl->create_opening_proof(scheme, reinterpret_cast<const typename K::Fr* const*>(polys), lens, num_polys,
                                      poly_idx, static_cast<const typename K::Fr*>(points),
                                      static_cast<const typename K::Fr*>(values), num_openings, t,
                                      static_cast<typename K::Aff*>(out_affine), cap, out_count)
               ? 1
               : 0;
  });
  GUARD_END
}

void tachyon_mi355x_kzg_last_open_timings(const tachyon_mi355x_kzg* p, float* out_ms) {
  GUARD_BEGIN KZG_DISPATCH(p, impl->last_open_timings(out_ms)); GUARD_END
}

int tachyon_mi355x_kzg_poly_linear_combination(int curve, const void* const* polys, const size_t* lens,
                                               const void* coeffs, size_t count, const void* d, void* out,
                                               size_t out_len) {
  GUARD_BEGIN
  FR_DISPATCH(curve, return linear_combination<Fr>(polys, lens, coeffs, count, d, out, out_len));
  GUARD_END
}

int tachyon_mi355x_kzg_poly_divide_by_roots(int curve, const void* poly, size_t len, const void* roots, size_t nroots,
                                            void* out_quotient, void* out_remainders) {
  GUARD_BEGIN
  FR_DISPATCH(curve, return divide_by_roots<Fr>(poly, len, roots, nroots, out_quotient, out_remainders));
  GUARD_END
}

int tachyon_mi355x_kzg_opening_plan(int curve, int scheme, const size_t* lens, size_t num_polys, size_t n,
                                    const size_t* poly_idx, const void* points, const void* values,
                                    size_t num_openings, uint64_t* out, size_t cap, size_t* out_words) {
  GUARD_BEGIN
  FR_DISPATCH(curve, return opening_plan<Fr>(scheme, lens, num_polys, n, poly_idx, points, values, num_openings, out,
                                             cap, out_words));
  GUARD_END
}

}  // extern "C"
