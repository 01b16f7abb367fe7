// KZG with a device-resident SRS (see kzg.h for the reference mapping).
#include "kzg.h"

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "../capi/kzg_open_validate.h"
#include "../field/curve_constants.h"
#include "../ntt/ntt.h"

namespace tachyon_amd::kzg {

namespace {

constexpr unsigned kBlock = 256;

template <class Curve>
struct Generator;
template <>
struct Generator<Bn254G1> {
  static constexpr const uint64_t* x = consts::bn254_g1::kXMont64;
  static constexpr const uint64_t* y = consts::bn254_g1::kYMont64;
};
template <>
struct Generator<Bls381G1> {
  static constexpr const uint64_t* x = consts::bls12_381_g1::kXMont64;
  static constexpr const uint64_t* y = consts::bls12_381_g1::kYMont64;
};

template <class F>
F from_words(const uint64_t* w) {
  F r;
  for (int i = 0; i < F::N; ++i) r.v[i] = (uint32_t)(w[i / 2] >> (32 * (i & 1)));
  return r;
}

// s_i = tau^i; l_i = L_i(tau) = (Z_H(tau) / n) * w^i / (tau - w^i)
// (EvaluatePartialLagrangeCoefficients, univariate_evaluation_domain.h:308-360,
// offset 1), one Fermat inverse per element
template <class Fr>
__global__ __launch_bounds__(kBlock) void srs_scalars_kernel(Fr tau, Fr omega, Fr z_over_n, uint32_t n,
                                                             Fr* __restrict__ s, Fr* __restrict__ l) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Fr ti = tau.pow(&i, 1);
  s[i] = ti.canonical();
  if (l) {
    const Fr wi = omega.pow(&i, 1);
    l[i] = (z_over_n * wi * (tau - wi).inverse()).canonical();
  }
}

// out_i = k_i * G (BatchMapScalarFieldToPoint), double-and-add from the top bit
template <class Curve>
__global__ __launch_bounds__(kBlock) void fixed_base_kernel(Affine<typename Curve::F> g,
                                                            const typename Curve::Fr* __restrict__ k, uint32_t n,
                                                            Affine<typename Curve::F>* __restrict__ out) {
  using F = typename Curve::F;
  using Fr = typename Curve::Fr;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Fr c = k[i].from_mont();
  XYZZ<F> r = XYZZ<F>::zero();
  for (int b = Fr::N * 32 - 1; b >= 0; --b) {
    r = r.dbl();
    if ((c.v[b / 32] >> (b % 32)) & 1) r = r.madd(g);
  }
  out[i] = r.to_affine();
}

}  // namespace

template <class Curve>
Kzg<Curve>::Kzg(hipStream_t stream) : stream_(stream) {
  require_gpu();
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  msm_ = std::make_unique<msm::MsmGpu<Curve>>(stream_);
}

template <class Curve>
Kzg<Curve>::~Kzg() {
  msm_.reset();
  if (own_stream_) (void)hipStreamDestroy(stream_);
}

template <class Curve>
void Kzg<Curve>::unsafe_setup(size_t size, const Fr& tau) {
  if (size == 0 || (size & (size - 1)) || size > (size_t(1) << 30))
    throw std::runtime_error("tachyon_mi355x: KZG setup size must be a power of two <= 2^30");
  uint32_t log_n = 0;
  while ((size_t(1) << log_n) < size) ++log_n;
  const Fr omega = ntt::root_of_unity<Fr>(log_n);
  const uint32_t n = (uint32_t)size;
  const uint32_t e = n;
  const Fr z = tau.pow(&e, 1) - Fr::one();  // Z_H(tau) = tau^n - 1
  Fr* d_s = static_cast<Fr*>(scratch_.ensure(2 * size * sizeof(Fr)));
  Fr* d_l = d_s + size;
  const unsigned grid = ceil_div(size, kBlock);
  if (!z.is_zero()) {
    const Fr z_over_n = z * ntt::field_from_u64<Fr>(size).inverse();
    hipLaunchKernelGGL(srs_scalars_kernel<Fr>, dim3(grid), dim3(kBlock), 0, stream_, tau, omega, z_over_n, n, d_s,
                       d_l);
  } else {
    // tau = w^j: L_j(tau) = 1, every other coefficient 0 (univariate_evaluation_domain.h:309-323)
    hipLaunchKernelGGL(srs_scalars_kernel<Fr>, dim3(grid), dim3(kBlock), 0, stream_, tau, omega, Fr::zero(), n, d_s,
                       static_cast<Fr*>(nullptr));
    std::vector<Fr> l(size, Fr::zero());
    Fr w = Fr::one();
    for (size_t j = 0; j < size; ++j, w = w * omega)
      if (w == tau) {
        l[j] = Fr::one();
        break;
      }
    TA_HIP(hipMemcpyAsync(d_l, l.data(), size * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    TA_HIP(hipStreamSynchronize(stream_));
  }
  TA_HIP(hipGetLastError());
  const Aff g{from_words<F>(Generator<Curve>::x), from_words<F>(Generator<Curve>::y)};
  Aff* d_p = static_cast<Aff*>(powers_.ensure(size * sizeof(Aff)));
  Aff* d_lg = static_cast<Aff*>(lagrange_.ensure(size * sizeof(Aff)));
  hipLaunchKernelGGL(fixed_base_kernel<Curve>, dim3(grid), dim3(kBlock), 0, stream_, g, d_s, n, d_p);
  hipLaunchKernelGGL(fixed_base_kernel<Curve>, dim3(grid), dim3(kBlock), 0, stream_, g, d_l, n, d_lg);
  TA_HIP(hipGetLastError());
  TA_HIP(hipStreamSynchronize(stream_));
  n_ = size;
}

template <class Curve>
bool Kzg<Curve>::downsize(size_t n) {
  if (n >= n_) return false;
  n_ = n;  // the device arrays keep their capacity; only the prefix is used
  return true;
}

template <class Curve>
bool Kzg<Curve>::commit(const Fr* scalars, size_t len, bool lagrange, Aff* out) {
  if (len > n_) return false;
  *out = msm_->run(d_srs(lagrange), scalars, len).to_affine();
  return true;
}

// XYZZ -> affine for a whole batch with one inversion: x = X / ZZ = X (ZZZ^-1 ZZ)^2,
// y = Y / ZZZ (point_xyzz.h:199-212), the ZZZ inverted together by
// Montgomery's trick (prefix products, one inverse, backward pass); identity
// points (zz = 0) stay (0, 0).
template <class F>
void batch_to_affine(const std::vector<XYZZ<F>>& pts, Affine<F>* out) {
  const size_t m = pts.size();
  std::vector<F> prefix(m);
  F acc = F::one();
  for (size_t i = 0; i < m; ++i) {
    if (!pts[i].is_zero()) acc = acc * pts[i].zzz;
    prefix[i] = acc;
  }
  F inv = acc.inverse();  // product of the non-identity ZZZ: invertible
  for (size_t i = m; i-- > 0;) {
    if (pts[i].is_zero()) {
      out[i] = Affine<F>::zero();
      continue;
    }
    const F zinv3 = i > 0 ? inv * prefix[i - 1] : inv;  // 1 / ZZZ_i
    inv = inv * pts[i].zzz;
    const F zinv2 = (zinv3 * pts[i].zz).sqr();
    out[i] = Affine<F>{pts[i].x * zinv2, pts[i].y * zinv3}.canonical();
  }
}

template <class Curve>
bool Kzg<Curve>::commit_batch(const Fr* const* scalars, const size_t* lens, size_t count, bool lagrange, Aff* out) {
  for (size_t i = 0; i < count; ++i)
    if (lens[i] > n_) return false;
  // Polynomials of similar length go into one batched MSM (MsmGpu::run_batch:
  // a block of windows per polynomial, one recode / sort / accumulation /
  // reduction) over the SRS prefix of the group's longest one, the others
  // zero-padded.  Groups are taken longest first and closed when padding
  // would more than double the group's work (count x L > 2 x sum of lens),
  // at run_batch's limits (max_batch_count) or at kGroupScalars padded
  // scalars (the batch's sort buffers grow ~16 B per scalar-window); a
  // group of one is a plain MSM.  So a ragged batch costs about its real
  // work, and a halo2-sized batch (thousands of columns of 2^20) runs as
  // several batched MSMs instead of one refused one.
  constexpr size_t kGroupScalars = size_t(1) << 26;
  std::vector<size_t> order;
  for (size_t i = 0; i < count; ++i)
    if (lens[i]) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return lens[a] > lens[b]; });
  std::vector<XYZZ<F>> pts(count, XYZZ<F>::zero());
  const Aff* srs = d_srs(lagrange);
  for (size_t i = 0; i < order.size();) {
    const size_t L = lens[order[i]];
    const size_t cap = std::min(msm_->max_batch_count(L), std::max<size_t>(1, kGroupScalars / L));
    size_t j = i + 1, sum = L;
    while (j < order.size() && j - i < cap && (j - i + 1) * L <= 2 * (sum + lens[order[j]])) sum += lens[order[j++]];
    const size_t g = j - i;
    if (g == 1) {
      pts[order[i]] = msm_->run(srs, scalars[order[i]], L);
    } else {
      Fr* padded = static_cast<Fr*>(batch_.ensure(g * L * sizeof(Fr)));
      TA_HIP(hipMemsetAsync(padded, 0, g * L * sizeof(Fr), msm_->stream()));
      for (size_t k = 0; k < g; ++k)  // host or device polynomials
        TA_HIP(hipMemcpyAsync(padded + k * L, scalars[order[i + k]], lens[order[i + k]] * sizeof(Fr),
                              hipMemcpyDefault, msm_->stream()));
      const auto res = msm_->run_batch(srs, padded, L, g);
      for (size_t k = 0; k < g; ++k) pts[order[i + k]] = res[k];
    }
    i = j;
  }
  batch_to_affine(pts, out);
  return true;
}

template <class Curve>
void Kzg<Curve>::copy_srs(bool lagrange, Aff* host_out) const {
  TA_HIP(hipMemcpy(host_out, d_srs(lagrange), n_ * sizeof(Aff), hipMemcpyDeviceToHost));
}

namespace {

// Coefficients of the interpolant of (x_k, y_k), k < n, the x_k distinct
// (math::LagrangeInterpolate): sum_k y_k prod_{i != k} (X - x_i) / (x_k - x_i)
template <class Fr>
std::vector<Fr> lagrange_interpolate(const std::vector<Fr>& x, const std::vector<Fr>& y) {
  const size_t n = x.size();
  std::vector<Fr> r(n, Fr::zero());
  for (size_t k = 0; k < n; ++k) {
    std::vector<Fr> num{Fr::one()};
    Fr den = Fr::one();
    for (size_t i = 0; i < n; ++i) {
      if (i == k) continue;
      num.push_back(Fr::zero());  // num *= (X - x_i)
      for (size_t j = num.size() - 1; j > 0; --j) num[j] = num[j - 1] - x[i] * num[j];
      num[0] = -(x[i] * num[0]);
      den = den * (x[k] - x[i]);
    }
    const Fr s = y[k] * den.inverse();
    for (size_t j = 0; j < n; ++j) r[j] = r[j] + s * num[j];
  }
  return r;
}

template <class Fr>
Fr horner(const std::vector<Fr>& p, const Fr& z) {
  Fr acc = Fr::zero();
  for (size_t j = p.size(); j-- > 0;) acc = p[j] + z * acc;
  return acc;
}

}  // namespace

template <class Curve>
bool Kzg<Curve>::evaluate_batch(const Fr* const* polys, const size_t* lens, size_t count, const size_t* idx,
                                const Fr* points, size_t m, Fr* out) {
  if (m != 0 && (!idx || !points || !out)) return false;
  if (count != 0 && (!polys || !lens)) return false;
  for (size_t i = 0; i < count; ++i)
    if (lens[i] != 0 && !polys[i]) return false;
  for (size_t i = 0; i < m; ++i)
    if (idx[i] >= count) return false;
  if (!poly_) poly_ = std::make_unique<PolyOps<Fr>>(stream_);
  PhaseClock timer(stream_);
  std::vector<const Fr*> dev;
  poly_->stage(polys, lens, count, &dev);
  std::vector<typename PolyOps<Fr>::Pair> pairs(m);
  for (size_t i = 0; i < m; ++i) pairs[i] = {dev[idx[i]], lens[idx[i]], points[i]};
  timer.begin(0);
  poly_->evaluate(pairs.data(), m, out);
  timer.end();
  poly_->synchronize();
  std::fill(open_ms_, open_ms_ + 4, 0.f);
  timer.sum(open_ms_, 4);
  return true;
}

template <class Curve>
bool Kzg<Curve>::create_opening_proof(int scheme, const Fr* const* polys, const size_t* lens, size_t count,
                                      const size_t* idx, const Fr* points, const Fr* values, size_t m,
                                      const Transcript& transcript, Aff* out, size_t cap, size_t* out_count) {
  using Term = typename PolyOps<Fr>::Term;
  if (!transcript.squeeze_challenge || !transcript.write_to_proof || !out_count || (cap != 0 && !out)) return false;
  kzg_open::Openings o;
  o.poly = idx;
  o.points = reinterpret_cast<const unsigned char*>(points);
  o.values = reinterpret_cast<const unsigned char*>(values);
  o.elem_bytes = sizeof(Fr);
  o.count = m;
  if (count != 0 && !polys) return false;
  kzg_open::Plan plan;
  if (!kzg_open::make_plan(scheme, o, lens, count, n_, element_less<Fr>, &plan)) return false;
  for (size_t i = 0; i < count; ++i)
    if (lens[i] != 0 && !polys[i]) return false;
  const size_t num_groups = plan.groups.size();
  if (cap < (scheme == kzg_open::kGwc ? num_groups : 2)) return false;
  // SHPlonk normalises by the first group's Z_{T\0}(u): nothing to open, no proof
  if (scheme == kzg_open::kShplonk && num_groups == 0) return false;

  if (!poly_) poly_ = std::make_unique<PolyOps<Fr>>(stream_);
  PhaseClock timer(stream_);
  std::vector<const Fr*> dev;
  poly_->stage(polys, lens, count, &dev);
  auto squeeze = [&] {
    Fr c;
    transcript.squeeze_challenge(transcript.ctx, &c);
    return c;
  };
  auto done = [&](bool ok) {
    poly_->synchronize();
    std::fill(open_ms_, open_ms_ + 4, 0.f);
    timer.sum(open_ms_, 4);
    return ok;
  };
  auto commit_and_write = [&](const std::vector<const Fr*>& ptrs, const std::vector<size_t>& qlens) {
    std::vector<Aff> affs(ptrs.size());
    timer.begin(3);
    const bool ok = commit_batch(ptrs.data(), qlens.data(), ptrs.size(), false, affs.data());
    timer.end();
    if (!ok) return false;
    for (const Aff& a : affs) {
      out[(*out_count)++] = a;
      if (!transcript.write_to_proof(transcript.ctx, &a)) return false;
    }
    return true;
  };
  *out_count = 0;
  // the longest polynomial of each group, and room for every group's quotient
  std::vector<size_t> glen(num_groups, 0), qlen(num_groups), qoff(num_groups);
  size_t quot_total = 0, num_len = 0, low_total = 0;
  for (size_t g = 0; g < num_groups; ++g) {
    const kzg_open::Group& grp = plan.groups[g];
    for (size_t p : grp.polys) glen[g] = std::max(glen[g], lens[p]);
    if (scheme == kzg_open::kShplonk) glen[g] = std::max(glen[g], grp.points.size());  // the interpolants
    qlen[g] = glen[g] - std::min(glen[g], grp.points.size());
    qoff[g] = quot_total;
    quot_total += qlen[g];
    low_total += grp.points.size();
    num_len = std::max(num_len, glen[g]);
  }
  Fr* quot = static_cast<Fr*>(open_quot_.ensure(std::max<size_t>(1, quot_total) * sizeof(Fr)));
  Fr* num = static_cast<Fr*>(open_num_.ensure(std::max<size_t>(1, num_len) * sizeof(Fr)));

  if (scheme == kzg_open::kGwc) {
    // W_g = (sum_j v^j P_j - sum_j v^j P_j(x_g)) / (X - x_g), j over the group's openings
    const Fr v = squeeze();
    std::vector<const Fr*> ptrs(num_groups);
    for (size_t g = 0; g < num_groups; ++g) {
      const kzg_open::Group& grp = plan.groups[g];
      std::vector<Term> terms;
      Fr c = Fr::one(), d = Fr::zero();
      for (size_t j = 0; j < grp.polys.size(); ++j, c = c * v) {
        terms.push_back({dev[grp.polys[j]], lens[grp.polys[j]], c});
        d = d + c * values[grp.values[j]];
      }
      timer.begin(1);
      poly_->linear_combination(terms.data(), terms.size(), d, num, glen[g]);
      timer.end();
      timer.begin(2);
      poly_->divide_by_roots(num, glen[g], &points[grp.points[0]], 1, quot + qoff[g], nullptr);
      timer.end();
      ptrs[g] = quot + qoff[g];
    }
    return done(commit_and_write(ptrs, qlen));
  }

  // SHPlonk.  R_j: the interpolant of polynomial j's claimed values on its
  // group's points; Rc_g = sum_j y^j R_j enters the numerator as one more
  // (low-degree) input with coefficient -1.
  const Fr y = squeeze();
  std::vector<std::vector<Fr>> group_points(num_groups);
  std::vector<std::vector<std::vector<Fr>>> interp(num_groups);
  std::vector<Fr> low(low_total);
  Fr* d_low = static_cast<Fr*>(open_low_.ensure(std::max<size_t>(1, low_total) * sizeof(Fr)));
  size_t low_off = 0;
  std::vector<size_t> low_offs(num_groups);
  for (size_t g = 0; g < num_groups; ++g) {
    const kzg_open::Group& grp = plan.groups[g];
    const size_t k = grp.points.size();
    for (size_t pt : grp.points) group_points[g].push_back(points[pt]);
    low_offs[g] = low_off;
    Fr c = Fr::one();
    for (size_t j = 0; j < grp.polys.size(); ++j, c = c * y) {
      std::vector<Fr> vals(k);
      for (size_t i = 0; i < k; ++i) vals[i] = values[grp.values[j * k + i]];
      interp[g].push_back(lagrange_interpolate(group_points[g], vals));
      for (size_t i = 0; i < k; ++i) low[low_off + i] = (j ? low[low_off + i] : Fr::zero()) + c * interp[g][j][i];
    }
    low_off += k;
  }
  if (low_total) TA_HIP(hipMemcpyAsync(d_low, low.data(), low_total * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  // H_g = (sum_j y^j P_j - Rc_g) / Z_g
  for (size_t g = 0; g < num_groups; ++g) {
    const kzg_open::Group& grp = plan.groups[g];
    std::vector<Term> terms;
    Fr c = Fr::one();
    for (size_t j = 0; j < grp.polys.size(); ++j, c = c * y) terms.push_back({dev[grp.polys[j]], lens[grp.polys[j]], c});
    terms.push_back({d_low + low_offs[g], grp.points.size(), -Fr::one()});
    timer.begin(1);
    poly_->linear_combination(terms.data(), terms.size(), Fr::zero(), num, glen[g]);
    timer.end();
    timer.begin(2);
    poly_->divide_by_roots(num, glen[g], group_points[g].data(), grp.points.size(), quot + qoff[g], nullptr);
    timer.end();
  }
  // H = sum_g v^g H_g
  const Fr v = squeeze();
  size_t h_len = 0;
  for (size_t g = 0; g < num_groups; ++g) h_len = std::max(h_len, qlen[g]);
  Fr* h = static_cast<Fr*>(open_h_.ensure(std::max<size_t>(1, 2 * num_len) * sizeof(Fr)));
  {
    std::vector<Term> terms;
    Fr c = Fr::one();
    for (size_t g = 0; g < num_groups; ++g, c = c * v) terms.push_back({quot + qoff[g], qlen[g], c});
    timer.begin(1);
    poly_->linear_combination(terms.data(), terms.size(), Fr::zero(), h, h_len);
    timer.end();
  }
  if (!commit_and_write({h}, {h_len})) return done(false);
  const Fr u = squeeze();
  // Z_{T \ g}(u) for every group, Z_T(u); everything is scaled by
  // 1 / Z_{T \ 0}(u) up front, so that Q = L / (X - u) needs no pass of its own
  std::vector<Fr> z_diff(num_groups, Fr::one());
  Fr z_t = Fr::one();
  for (size_t s : plan.super_points) {
    const Fr f = u - points[s];
    z_t = z_t * f;
    for (size_t g = 0; g < num_groups; ++g)
      if (std::find(plan.groups[g].points.begin(), plan.groups[g].points.end(), s) == plan.groups[g].points.end())
        z_diff[g] = z_diff[g] * f;
  }
  if (z_diff[0].is_zero()) return done(false);
  const Fr inv0 = z_diff[0].inverse();
  // L = sum_g v^g Z_{T\g}(u) sum_j y^j (P_j - R_j(u)) - Z_T(u) H
  std::vector<Term> terms;
  Fr d = Fr::zero(), vg = Fr::one();
  size_t l_len = h_len;
  for (size_t g = 0; g < num_groups; ++g, vg = vg * v) {
    const kzg_open::Group& grp = plan.groups[g];
    const Fr scale = vg * z_diff[g] * inv0;
    Fr c = scale;
    for (size_t j = 0; j < grp.polys.size(); ++j, c = c * y) {
      terms.push_back({dev[grp.polys[j]], lens[grp.polys[j]], c});
      d = d + c * horner(interp[g][j], u);
      l_len = std::max(l_len, lens[grp.polys[j]]);
    }
  }
  terms.push_back({h, h_len, -(z_t * inv0)});
  Fr* q = h + num_len;  // the second half of the buffer
  timer.begin(1);
  poly_->linear_combination(terms.data(), terms.size(), d, num, l_len);
  timer.end();
  timer.begin(2);
  poly_->divide_by_roots(num, l_len, &u, 1, q, nullptr);
  timer.end();
  return done(commit_and_write({q}, {l_len ? l_len - 1 : 0}));
}

template class Kzg<Bn254G1>;
template class Kzg<Bls381G1>;

}  // namespace tachyon_amd::kzg
