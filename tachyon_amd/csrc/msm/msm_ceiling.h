// MsmGpu::madd_ceiling: the accumulation's madd in registers, kernels and host timing
// (part of msm_impl.h).
#pragma once

namespace tachyon_amd::msm {

// The accumulation's madd in registers: a chain of `iters` additions of one
// point per thread (no gathers, no bucket runs, 3 waves per SIMD as the
// accumulation kernels).  The result is stored so nothing is dead code.
namespace detail {
namespace {
__global__ __launch_bounds__(kBlock, 3) void madd_ceiling29_kernel(const Affine<Bn254Fq>* __restrict__ pts,
                                                                   XYZZ<Bn254Fq>* __restrict__ out, int iters) {
  using namespace acc29;
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const Affine<Bn254Fq> p = pts[t & 1023], q = pts[(t + 5) & 1023];
  const F29 x2 = shl5_repack(q.x.v), y2 = shl5_repack(q.y.v);
  Acc acc = from_shifted(shl5_repack(p.x.v), shl5_repack(p.y.v));
  int special = 0;
  for (int i = 0; i < iters; ++i) acc = madd(acc, x2, y2, &special);
  XYZZ<Bn254Fq> r = to_xyzz(acc);
  r.zz.v[0] ^= (uint32_t)special;
  out[t] = r;
}
__global__ __launch_bounds__(kBlock, 3) void madd_ceiling32_kernel(const Affine<Bn254Fq>* __restrict__ pts,
                                                                   XYZZ<Bn254Fq>* __restrict__ out, int iters) {
  using F = HotFp<Bn254Fq>;
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const Affine<F> p{pts[t & 1023].x, pts[t & 1023].y}, q{pts[(t + 5) & 1023].x, pts[(t + 5) & 1023].y};
  XYZZ<F> acc{p.x, p.y, F::one(), F::one()};
  bool zero = false;
  for (int i = 0; i < iters; ++i) acc = acc.madd_nz(q, &zero);
  out[t] = XYZZ<Bn254Fq>{acc.x, acc.y, zero ? Bn254Fq::zero() : Bn254Fq(acc.zz), acc.zzz};
}
// ... BLS12-381 G1's 14 x 28-bit field (Pol28), at seg_acc28_kernel's 2 waves per SIMD
__global__ __launch_bounds__(kBlock, 2) void madd_ceiling28_kernel(const Affine<Bls381Fq>* __restrict__ pts,
                                                                   XYZZ<Bls381Fq>* __restrict__ out, int iters) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const Affine<Bls381Fq> p = pts[t & 1023], q = pts[(t + 5) & 1023];
  const Pol28::F x2 = Pol28::shift_repack(q.x.v), y2 = Pol28::shift_repack(q.y.v);
  Pol28::Acc acc = Pol28::from_shifted(Pol28::shift_repack(p.x.v), Pol28::shift_repack(p.y.v));
  int special = 0;
  for (int i = 0; i < iters; ++i) acc = Pol28::madd(acc, x2, y2, &special);
  XYZZ<Bls381Fq> r = Pol28::to_xyzz(acc);
  r.zz.v[0] ^= (uint32_t)special;
  out[t] = r;
}
// ... the G2 lane pairs over the limb fields (PairPol28 / PairPol29, as
// seg_acc_pair_limb_kernel): lane h of a pair holds component h; pts are Fq2
// affine points as 4 base-field components (x0 x1 y0 y1)
template <class Pol>
__global__ __launch_bounds__(kBlock) void madd_ceiling_pair_kernel(const typename Pol::Fb* __restrict__ comps,
                                                                   typename Pol::Fb* __restrict__ out, int iters) {
  using Fb = typename Pol::Fb;
  const uint32_t h = threadIdx.x & 1u;
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const int pair = t >> 1;
  const Fb* p = comps + 4 * (pair & 1023);
  const Fb* q = comps + 4 * ((pair + 5) & 1023);
  const typename Pol::F x2 = Pol::repack(q[h].v), y2 = Pol::repack(q[2 + h].v);
  typename Pol::Acc acc = Pol::start(Pol::repack(p[h].v), Pol::repack(p[2 + h].v), h != 0);
  int special = 0;
  for (int i = 0; i < iters; ++i) acc = Pol::madd(acc, x2, y2, h != 0, &special);
  Fb v;
  Pol::to32(acc.x, v.v);
  v.v[0] ^= (uint32_t)special;
  out[4 * (size_t)t] = v;
  Pol::to32(acc.y, v.v);
  out[4 * (size_t)t + 1] = v;
  Pol::to32(acc.zz, v.v);
  out[4 * (size_t)t + 2] = v;
  Pol::to32(acc.zzz, v.v);
  out[4 * (size_t)t + 3] = v;
}

// Best-of-3 rate (G additions/s) of a ceiling kernel over `pts_words`
// pseudo-random field words below the modulus (not curve points: the formula
// does not care), `lanes_per_add` lanes per addition
template <class In, class Out, class Kern>
double time_ceiling(Kern kern, size_t in_words, size_t out_bytes_per_thread, unsigned top_mask_words,
                    uint32_t top_mask, unsigned lanes_per_add) {
  constexpr int kBlocks = 256 * 12, kIters = 400;
  std::vector<uint32_t> h(in_words);
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (size_t i = 0; i < h.size(); ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    h[i] = (uint32_t)(s >> 32);
    if (i % top_mask_words == top_mask_words - 1) h[i] &= top_mask;  // the top word of each element
  }
  void* pts = nullptr;
  void* out = nullptr;
  hipEvent_t e0, e1;
  TA_HIP(hipMalloc(&pts, h.size() * 4));
  TA_HIP(hipMalloc(&out, (size_t)kBlocks * kBlock * out_bytes_per_thread));
  TA_HIP(hipMemcpy(pts, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  TA_HIP(hipEventCreate(&e0));
  TA_HIP(hipEventCreate(&e1));
  hipLaunchKernelGGL(kern, dim3(kBlocks), dim3(kBlock), 0, 0, static_cast<const In*>(pts), static_cast<Out*>(out), 4);
  float best = 1e30f;
  for (int r = 0; r < 3; ++r) {
    TA_HIP(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(kern, dim3(kBlocks), dim3(kBlock), 0, 0, static_cast<const In*>(pts), static_cast<Out*>(out),
                       kIters);
    TA_HIP(hipEventRecord(e1, 0));
    TA_HIP(hipEventSynchronize(e1));
    float ms = 0;
    TA_HIP(hipEventElapsedTime(&ms, e0, e1));
    best = std::min(best, ms);
  }
  TA_HIP(hipGetLastError());
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(pts);
  (void)hipFree(out);
  return (double)kBlocks * kBlock / lanes_per_add * kIters / (best * 1e-3) / 1e9;
}
}  // namespace
}  // namespace detail

template <class Curve>
double MsmGpu<Curve>::madd_ceiling(int field_bits) {
  using namespace detail;
  if constexpr (std::is_same_v<Curve, Bn254G1>) {
    if (field_bits != 29 && field_bits != 32) return 0.0;
    require_gpu();
    auto* kern = field_bits == 29 ? &madd_ceiling29_kernel : &madd_ceiling32_kernel;
    return time_ceiling<Affine<Bn254Fq>, XYZZ<Bn254Fq>>(kern, 1024 * 16, sizeof(XYZZ<Bn254Fq>), 8, 0x0fffffffu, 1);
  } else if constexpr (std::is_same_v<Curve, Bls381G1>) {
    if (field_bits != 28) return 0.0;
    require_gpu();
    return time_ceiling<Affine<Bls381Fq>, XYZZ<Bls381Fq>>(&madd_ceiling28_kernel, 1024 * 24, sizeof(XYZZ<Bls381Fq>), 12, 0x0fffffffu, 1);
  } else if constexpr (std::is_same_v<Curve, Bls381G2>) {
    if (field_bits != 28) return 0.0;
    require_gpu();
    return time_ceiling<Bls381Fq, Bls381Fq>(&madd_ceiling_pair_kernel<PairPol28>, 1024 * 48, 4 * sizeof(Bls381Fq), 12,
                                  0x0fffffffu, 2);
  } else {
    if (field_bits != 29) return 0.0;
    require_gpu();
    return time_ceiling<Bn254Fq, Bn254Fq>(&madd_ceiling_pair_kernel<PairPol29>, 1024 * 32, 4 * sizeof(Bn254Fq), 8,
                                 0x0fffffffu, 2);
  }
}

}  // namespace tachyon_amd::msm
