// MSM bases: non-affine inputs to affine, and the fold tables (part of msm_impl.h).
#pragma once

namespace tachyon_amd::msm {
namespace detail {
namespace {  // internal linkage: every per-curve TU gets its own copy

// ---------------------------------------------------------------------------
// Non-affine bases -> affine (VariableBaseMSM<ProjectivePoint / JacobianPoint /
// PointXYZZ>, variable_base_msm_unittest.cc:30-33): Montgomery's trick per
// thread over `chunk` consecutive points -- the denominators' prefix products
// to `prefix`, one inversion, then the backward pass.  form 1 projective
// {X, Y, Z}: (X/Z, Y/Z); 2 Jacobian {X, Y, Z}: (X/Z^2, Y/Z^3); 3 XYZZ
// {X, Y, ZZ, ZZZ}: (X (ZZ/ZZZ)^2, Y/ZZZ) (point_xyzz.h:199-212, ZZ^3 = ZZZ^2).
// A zero denominator is the identity -> (0, 0).  Canonical outputs.
template <class F>
__global__ __launch_bounds__(kBlock) void points_to_affine_kernel(const F* __restrict__ in, int form,
                                                                  Affine<F>* __restrict__ out,
                                                                  F* __restrict__ prefix, size_t n, uint32_t chunk) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t s = t * chunk;
  if (s >= n) return;
  const size_t e = s + chunk < n ? s + chunk : n;
  const unsigned stride = form == 3 ? 4 : 3;  // coordinates per input point
  const unsigned den = form == 3 ? 3 : 2;     // the denominator's coordinate
  F prod = F::one();
  for (size_t i = s; i < e; ++i) {
    const F d = in[i * stride + den];
    if (!d.is_zero()) prod = prod * d;
    prefix[i] = prod;
  }
  F inv = prod.inverse();  // product of the non-zero denominators
  for (size_t i = e; i-- > s;) {
    const F* p = in + i * stride;
    const F d = p[den];
    if (d.is_zero()) {
      out[i] = Affine<F>::zero();
      continue;
    }
    const F dinv = i > s ? inv * prefix[i - 1] : inv;
    inv = inv * d;
    Affine<F> a;
    if (form == 1) {
      a = {p[0] * dinv, p[1] * dinv};
    } else if (form == 2) {
      const F d2 = dinv.sqr();
      a = {p[0] * d2, p[1] * (d2 * dinv)};
    } else {
      a = {p[0] * (p[2] * dinv).sqr(), p[1] * dinv};
    }
    out[i] = a.canonical();
  }
}

// Folded bases (MsmGpu::fold_bases): copy k of point i = 2^(k shift) P_i as
// XYZZ (x, y, zz, zzz words) at out[(k n + i) * 4], by k shift doublings of
// one thread; points_to_affine_kernel (form 3) then normalises them.  A
// one-time table build (a proving key's), not a per-MSM pass.
template <class F>
__global__ __launch_bounds__(kBlock) void fold_points_kernel(const Affine<F>* __restrict__ in, size_t n, unsigned fold,
                                                             unsigned shift, F* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  XYZZ<F> p = XYZZ<F>::from_affine(in[i]);
  for (unsigned k = 0; k < fold; ++k) {
    if (k > 0)
      for (unsigned d = 0; d < shift; ++d) p = p.dbl();
    F* o = out + ((size_t)k * n + i) * 4;
    o[0] = p.x;
    o[1] = p.y;
    o[2] = p.zz;
    o[3] = p.zzz;
  }
}

}  // namespace
}  // namespace detail
}  // namespace tachyon_amd::msm
