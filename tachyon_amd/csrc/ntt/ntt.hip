// Radix-2 NTT for MI355X (gfx950): the host drivers NttDomain, NttGenDomain,
// Ntt4Step and NttMultiDevice.  Their kernels are in the three headers below,
// one translation unit with this file; one pass loop (run_passes) launches
// the passes of every transform.
// Reference semantics: radix2_evaluation_domain.h:213-333,
// univariate_evaluation_domain.h:141-232,464-489,518-566, radix2_twiddle_cache.h:57-121.
#include "ntt.h"

#include "ntt_pass32.h"
#include "ntt_pass29.h"
#include "ntt_tables.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <stdexcept>
#include <type_traits>

namespace tachyon_amd::ntt {

namespace {

template <class Fr>
Fr fr_from_u64(uint64_t v) {
  Fr x = Fr::zero();
  x.v[0] = (uint32_t)v;
  x.v[1] = (uint32_t)(v >> 32);
  return x.to_mont();
}

// halo2curves' BN254 Fr two-adic root of unity 7^((r-1)/2^28), Montgomery limbs
// exactly as OverrideSubgroupGenerator writes kTwoAdicRootOfUnity
// (bn/bn254/halo2/bn254.cc:18-23).  GetRootOfUnity's large-subgroup branch
// (large^(3^2), bn254.cc:24-29) lands on the same element.
constexpr uint64_t kBn254FrHalo2TwoAdicRootMont64[4] = {10822932506504462008ULL, 10978899855858987673ULL,
                                                        12888607242213977304ULL, 2119232853909229097ULL};
std::atomic<bool> g_bn254_fr_halo2{false};

template <class Fr>
Fr two_adic_root() {
  Fr r;
  const uint64_t* src = Fr::Config::kTwoAdicRootMont64;
  if constexpr (std::is_same_v<Fr, Bn254Fr>) {
    if (g_bn254_fr_halo2.load()) src = kBn254FrHalo2TwoAdicRootMont64;
  }
  for (int i = 0; i < Fr::N / 2; ++i) {
    r.v[2 * i] = (uint32_t)src[i];
    r.v[2 * i + 1] = (uint32_t)(src[i] >> 32);
  }
  return r;
}

// Pass plan of a 2^log_n-point transform: ceil(L / max_stages) passes, stages
// split evenly, as many sets per workgroup as lds_elems hold
template <class Pass>
std::vector<Pass> pass_plan(uint32_t log_n, uint32_t lds_elems, uint32_t max_stages) {
  std::vector<Pass> plan;
  if (log_n == 0) return plan;
  uint32_t P = (log_n + max_stages - 1) / max_stages;
  uint32_t s0 = 0;
  for (uint32_t p = 0; p < P; ++p) {
    uint32_t k = (log_n - s0) / (P - p);
    Pass ps;
    ps.s0 = s0;
    ps.k = k;
    ps.final_pass = (s0 + k == log_n);
    uint32_t avail = ps.final_pass ? (log_n - k) : (log_n - s0 - k);  // log2 of sets available
    uint32_t log_m = 0;
    while (log_m < avail && ((2u << log_m) << k) <= lds_elems) ++log_m;
    ps.log_m = log_m;
    plan.push_back(ps);
    s0 += k;
  }
  return plan;
}

template <class Fr>
std::vector<Fr> host_powers(const Fr& base, const Fr& scale, size_t count) {
  std::vector<Fr> out(count);
  Fr p = scale;
  for (size_t i = 0; i < count; ++i) {
    out[i] = p;
    p = p * base;
  }
  return out;
}

// ---------------------------------------------------------------------------
// The pass driver: every transform of NttDomain and NttGenDomain is one call
// of run_passes with the tables (32-bit or 29-bit) its passes read.

// A one-pass transform (<= 8 stages) smaller than a tile of kMaxLdsElems: 2^p
// batch entries per workgroup (the largest p with 2^p | batch and 2^(log_m + p)
// elements in the tile) instead of one entry using 2^log_m / 4 of its 256
// threads -- the 2^8-point column NTTs of the four-step's 2^8 x 2^16 split.
uint32_t pack_log(size_t passes, uint32_t log_m, size_t batch) {
  if (passes != 1 || batch < 2) return 0;
  uint32_t p = 0;
  while (batch % (size_t(2) << p) == 0 && ((size_t(1) << log_m) << (p + 1)) <= kMaxLdsElems) ++p;
  return p;
}

// The two-level power tables of a coset offset: lo / hi of the forward load,
// ilo / ihi of the inverse store (the size's inverse included)
template <class Fr>
struct CosetPtrs {
  const Fr* lo;
  const Fr* hi;
  const Fr* ilo;
  const Fr* ihi;
};

// PassArgs of pass `ps` of a 2^L-point transform (first: its first pass).
// c = the coset's power tables (null: the plain domain), fs = the four-step
// exchange fused into the first / last pass (null: the batched layout)
template <class Fr, class Pass>
PassArgs<Fr> pass_args(const Pass& ps, uint32_t L, bool first, bool inverse, const Fr& size_inv,
                       const CosetPtrs<Fr>* c, const FourStepTw<Fr>* fs, uint32_t pack) {
  PassArgs<Fr> a{};
  a.L = L;
  a.s0 = ps.s0;
  a.k = ps.k;
  a.log_m = pack ? pack : ps.log_m;
  a.final_pass = ps.final_pass ? 1u : 0u;
  a.pow_bits = (L + 1) / 2;
  a.mode = 0;
  if (first && !inverse && c) {
    a.mode |= kLoadCoset;
    a.load_lo = c->lo;
    a.load_hi = c->hi;
  }
  if (ps.final_pass && inverse) {
    if (c) {
      a.mode |= kStoreCoset;
      a.store_lo = c->ilo;
      a.store_hi = c->ihi;
    } else {
      a.mode |= kStoreScale;
      a.scale = size_inv;
    }
  }
  if (fs) {
    a.fs = *fs;
    if (fs->rows) {
      if (first && !inverse) a.mode |= kLoadXch;
      if (ps.final_pass && inverse) a.mode |= kStoreXch;
    } else {
      if (first && inverse) a.mode |= kLoadTw4;
      if (ps.final_pass && !inverse) a.mode |= kStoreTw4;
    }
  }
  a.pack = pack;
  return a;
}

// The stage tables of the 32-bit passes (dif_pass_kernel) in one direction.
// Shoup twiddles (64 B) in the passes whose stage tables are small and
// cache-resident; Montgomery twiddles (32 B) where the tables stream from HBM
// -- the first pass reads the big tables of stages 0.. once each.
template <class Fr>
struct Tables32 {
  using Tw = typename NttTw<Fr>::type;
  static constexpr bool kShoup = !std::is_same_v<Tw, Fr>;
  const Tw* tw;        // the Shoup entries (fields without them: the Montgomery tables, as twm)
  const Fr* twm;       // the Montgomery twiddles
  int shoup_mode = 2;  // Shoup twiddles: 0 never, 1 every pass, 2 all but the first pass
  // tuning builds only: DIF stages per register step, and the A/B kernels (bit
  // 0 = the Montgomery radix-4 pass at >= 5 waves/SIMD, bit 1 = the Shoup
  // radix-4 passes without the twiddle prefetch at >= 5 waves/SIMD)
  int radix = 2, ab = 0;

  void launch(size_t p, dim3 grid, uint32_t elems, hipStream_t stream, const void* src, void* dst,
              const PassArgs<Fr>& a) const {
    const Fr* in = static_cast<const Fr*>(src);
    Fr* out = static_cast<Fr*>(dst);
    const size_t lds = (size_t)elems * sizeof(Fr);
    const bool shoup = kShoup && (shoup_mode == 1 || (shoup_mode == 2 && p > 0));
#ifdef TACHYON_TUNING_KNOBS
    // tiles above 64 KiB (TACHYON_NTT_LDS_ELEMS > 2048) need the kernel's dynamic-LDS limit raised
    auto allow = [&](const void* k) {
      if (lds > 64 * 1024) TA_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    };
    if (shoup) {
      auto kern = radix == 1 ? dif_pass_kernel<Fr, Tw, 1> : radix == 2 ? dif_pass_kernel<Fr, Tw, 2>
                                                                       : dif_pass_kernel<Fr, Tw, 3>;
      if (radix == 2 && (ab & 2)) kern = dif_pass_kernel<Fr, Tw, 2, false, 5>;
      allow(reinterpret_cast<const void*>(kern));
      hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, stream, in, out, tw, a);
    } else {
      auto kern = radix == 1 ? dif_pass_kernel<Fr, Fr, 1> : radix == 2 ? dif_pass_kernel<Fr, Fr, 2>
                                                                       : dif_pass_kernel<Fr, Fr, 3>;
      if (radix == 2 && (ab & 1)) kern = dif_pass_kernel<Fr, Fr, 2, true, 5>;
      allow(reinterpret_cast<const void*>(kern));
      hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, stream, in, out, twm, a);
    }
#else
    // release schedule: radix-4 register steps (2 DIF stages per LDS round trip)
    if (lds > 64 * 1024) throw std::runtime_error("tachyon_mi355x: NTT pass tile above 64 KiB in a release build");
    if (shoup) hipLaunchKernelGGL((dif_pass_kernel<Fr, Tw, 2>), grid, dim3(kBlock), lds, stream, in, out, tw, a);
    else hipLaunchKernelGGL((dif_pass_kernel<Fr, Fr, 2>), grid, dim3(kBlock), lds, stream, in, out, twm, a);
#endif
  }
};

// The tables of the 29-bit passes (dif29_pass_kernel, BN254 Fr) in one
// direction: R'-form entries for the first pass, Shoup entries (the stage
// tables from entry ts_off on) for the later ones.  Elements between passes
// are 36-byte F29: the scratch of these passes holds batch * 2^L of them.
// (Fr = Bn254Fr.  A template so that its kernels are instantiated with its
// callers, after Tables32's: the order of the kernels in the code object.)
template <class Fr>
struct Tables29 {
  const fr29::TwMont29* tm;
  const fr29::TwShoup29* ts;
  uint32_t ts_off;
  bool swizzle;  // XOR-swizzled LDS positions (swz29)

  void launch(size_t p, dim3 grid, uint32_t elems, hipStream_t stream, const void* src, void* dst,
              const PassArgs<Fr>& a) const {
    // the kernel's LDS planes are sized for kMaxLdsElems (tuning plans with larger tiles: 32-bit only)
    if (elems > kMaxLdsElems) throw std::runtime_error("tachyon_mi355x: 29-bit NTT pass tile above its LDS planes");
    if (p == 0) {
      auto* k0 = swizzle ? &dif29_pass_kernel<true, true, fr29::TwMont29> : &dif29_pass_kernel<true, false, fr29::TwMont29>;
      hipLaunchKernelGGL(k0, grid, dim3(kBlock), 0, stream, src, dst, Tw29Table<fr29::TwMont29>{tm, 0u}, a);
    } else {
      auto* k1 = swizzle ? &dif29_pass_kernel<false, true, fr29::TwShoup29>
                         : &dif29_pass_kernel<false, false, fr29::TwShoup29>;
      hipLaunchKernelGGL(k1, grid, dim3(kBlock), 0, stream, src, dst, Tw29Table<fr29::TwShoup29>{ts, ts_off}, a);
    }
  }
};

// The passes of `plan` over `batch` arrays of 2^L elements, enqueued on
// `stream`: the first pass reads src (null: data), the middle passes work in
// place on scratch, the final pass writes data -- a one-pass transform never
// touches scratch.  ev (null: no profile): plan.size() + 1 events, recorded
// before the first pass and after each one.
template <class Fr, class Tables, class Pass>
void run_passes(const Tables& tables, const std::vector<Pass>& plan, uint32_t L, bool inverse, size_t batch,
                uint32_t pack, const Fr& size_inv, const CosetPtrs<Fr>* coset, const FourStepTw<Fr>* fs,
                const Fr* src, Fr* data, void* scratch, hipStream_t stream, const hipEvent_t* ev) {
  if (ev) TA_HIP(hipEventRecord(ev[0], stream));
  for (size_t p = 0; p < plan.size(); ++p) {
    const Pass& ps = plan[p];
    const PassArgs<Fr> a = pass_args(ps, L, p == 0, inverse, size_inv, coset, fs, pack);
    const void* in = p == 0 ? static_cast<const void*>(src ? src : data) : scratch;
    void* out = ps.final_pass ? static_cast<void*>(data) : scratch;
    const uint32_t elems = (1u << a.log_m) << ps.k;
    const uint32_t blocks = pack ? 1u : (uint32_t)((size_t(1) << L) / elems);
    const uint32_t gy = (uint32_t)(batch >> pack);
    tables.launch(p, dim3(blocks, gy), elems, stream, in, out, a);
    TA_HIP(hipGetLastError());
    if (ev) TA_HIP(hipEventRecord(ev[p + 1], stream));
  }
}

}  // namespace

template <class Fr>
NttDomain<Fr>::NttDomain(size_t num_coeffs, hipStream_t stream) : stream_(stream) {
  require_gpu();
  log_n_ = 0;
  while ((size_t(1) << log_n_) < std::max<size_t>(num_coeffs, 1)) ++log_n_;
  if (log_n_ > (uint32_t)Fr::Config::kTwoAdicity || log_n_ > 30)
    throw std::runtime_error("tachyon_mi355x: NTT size exceeds the field's two-adicity");
  n_ = size_t(1) << log_n_;
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  // w_n = root^(2^(s - log n))  (PrimeFieldBase::GetRootOfUnity, prime_field_base.h:90-130)
  Fr omega = two_adic_root<Fr>();
  for (uint32_t i = log_n_; i < (uint32_t)Fr::Config::kTwoAdicity; ++i) omega = omega.sqr();
  setup(omega, true);
}

template <class Fr>
NttDomain<Fr>::NttDomain(const Fr& group_gen, uint32_t log_n, hipStream_t stream) : stream_(stream) {
  require_gpu();
  if (log_n > (uint32_t)Fr::Config::kTwoAdicity || log_n > 30)
    throw std::runtime_error("tachyon_mi355x: NTT size exceeds the field's two-adicity");
  log_n_ = log_n;
  n_ = size_t(1) << log_n_;
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  setup(group_gen, false);
}

// The domain generated by omega (order n_): constants, pass plan and tables
template <class Fr>
void NttDomain<Fr>::setup(const Fr& omega, bool default_variant) {
  omega_ = omega;
  omega_inv_ = omega_.inverse();
  size_inv_ = fr_from_u64<Fr>(n_).inverse();
  offset_ = Fr::one();
  offset_inv_ = Fr::one();

  // elements per workgroup (LDS footprint); TACHYON_NTT_LDS_ELEMS overrides it
  // in tuning builds only (-DTACHYON_TUNING_KNOBS, tools/tune_ntt.py)
  uint32_t lds_elems = kMaxLdsElems;
  uint32_t max_stages = kMaxPassStages;
#ifdef TACHYON_TUNING_KNOBS
  if (const char* e = getenv("TACHYON_NTT_LDS_ELEMS")) lds_elems = std::clamp<uint32_t>(atoi(e), 256, 4096);
  // (A/B of fewer, longer passes: 12 stages with 4096-element tiles = the
  // 2-pass 2^12 x 2^12 plan of 2^24, 128 KiB of LDS per workgroup)
  if (const char* e = getenv("TACHYON_NTT_PASS_STAGES")) max_stages = std::clamp<uint32_t>(atoi(e), 4, 12);
#endif
  plan_ = pass_plan<Pass>(log_n_, lds_elems, max_stages);
  pow_bits_ = (log_n_ + 1) / 2;
  // stages per register step (1 = radix-2 through LDS every stage) and the
  // other schedule overrides: A/B measurements in tuning builds only
#ifdef TACHYON_TUNING_KNOBS
  if (const char* e = getenv("TACHYON_NTT_RADIX_LOG")) radix_ = std::clamp(atoi(e), 1, 3);
  if (const char* e = getenv("TACHYON_NTT_SHOUP")) shoup_mode_ = std::clamp(atoi(e), 0, 2);
  if (const char* e = getenv("TACHYON_NTT_VARIANT")) ntt_variant_ = std::clamp(atoi(e), 0, 3);
#endif
  ev_.resize(plan_.size() + 1);
  for (auto& e : ev_) TA_HIP(hipEventCreate(&e));
  build_twiddles();
  // BN254 Fr up to 2^20: the 29-bit passes by default -- fewer instructions
  // win while the clock holds (2^20 forward 0.126 -> 0.118 ms, inverse 0.133 ->
  // 0.127); from 2^22 the 32-bit ones are faster (2^24 1.78 vs 1.88 ms
  // forward; profiles/r04b/ntt_ab_32_vs_29_2_20_24.log).  set_variant(0)
  // forces the 32-bit passes.
  if constexpr (std::is_same_v<Fr, Bn254Fr>) {
    if (default_variant && log_n_ >= 1 && log_n_ <= 20) {
      variant_ = 1;
      build_tables29();
    }
  }
}

template <class Fr>
NttDomain<Fr>::~NttDomain() {
  for (auto& e : ev_) (void)hipEventDestroy(e);
  if (own_stream_) (void)hipStreamDestroy(stream_);
}

template <class Fr>
void NttDomain<Fr>::build_twiddles() {
  if (log_n_ == 0) return;
  const uint32_t half = (uint32_t)(n_ / 2);
  const uint32_t lb = (log_n_ - 1 + 1) / 2;  // lo bits of the base table split
  const size_t lo_cnt = size_t(1) << lb;
  const size_t hi_cnt = std::max<size_t>(1, half >> lb);
  using Tw = typename NttTw<Fr>::type;
  constexpr bool kShoup = !std::is_same_v<Tw, Fr>;
  // Montgomery stage tables (stage s holds w^(j 2^s), j < n / 2^(s+1), at
  // offset n - (n >> s)): the twiddles of the 32-bit passes for fields without
  // Shoup entries, and the source of every other table (BN254 Fr: the 29-bit
  // tables now, the 32-bit Shoup ones on first use of set_variant bit 0)
  Fr* monts[2] = {kShoup ? static_cast<Fr*>(twm_fwd_.ensure(n_ * sizeof(Fr)))
                         : static_cast<Fr*>(tw_fwd_.ensure(n_ * sizeof(Tw))),
                  kShoup ? static_cast<Fr*>(twm_inv_.ensure(n_ * sizeof(Fr)))
                         : static_cast<Fr*>(tw_inv_.ensure(n_ * sizeof(Tw)))};
  DeviceBuffer lo_d, hi_d;
  Fr* lo = static_cast<Fr*>(lo_d.ensure(lo_cnt * sizeof(Fr)));
  Fr* hi = static_cast<Fr*>(hi_d.ensure(hi_cnt * sizeof(Fr)));
  for (int dir = 0; dir < 2; ++dir) {
    Fr w = dir == 0 ? omega_ : omega_inv_;
    std::vector<Fr> lo_h = host_powers(w, Fr::one(), lo_cnt);
    Fr w_step = w;
    for (uint32_t i = 0; i < lb; ++i) w_step = w_step.sqr();
    std::vector<Fr> hi_h = host_powers(w_step, Fr::one(), hi_cnt);
    TA_HIP(hipMemcpyAsync(lo, lo_h.data(), lo_cnt * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    TA_HIP(hipMemcpyAsync(hi, hi_h.data(), hi_cnt * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    Fr* mont = monts[dir];
    hipLaunchKernelGGL(twiddle_base_kernel<Fr>, dim3(ceil_div(half, kBlock)), dim3(kBlock), 0, stream_, mont, half,
                       lo, hi, lb);
    for (uint32_t s = 1; s < log_n_; ++s) {
      uint32_t cnt = (uint32_t)(n_ >> (s + 1));
      hipLaunchKernelGGL(twiddle_stage_kernel<Fr>, dim3(ceil_div(cnt, kBlock)), dim3(kBlock), 0, stream_,
                         mont + (n_ - (n_ >> s)), mont, cnt, s);
    }
    TA_HIP(hipGetLastError());
    TA_HIP(hipStreamSynchronize(stream_));  // host vectors go out of scope
  }
  if constexpr (kShoup) ensure_tables32();  // (the 29-bit tables are built on first use of variant bit 0)
}

// BN254 Fr: the 29-bit tables from the Montgomery stage tables (tw29_table_kernel)
template <class Fr>
void NttDomain<Fr>::build_tables29() {
  if constexpr (std::is_same_v<Fr, Bn254Fr>) {
    if (tables29_ || log_n_ == 0) return;
    tables29_ = true;
    const uint32_t k0 = plan_.empty() ? log_n_ : plan_[0].k;
    const size_t count = n_ - 1;  // all stage tables
    split29_ = n_ - (n_ >> k0);
    const size_t nshoup = count - split29_;
    DeviceBuffer* bm[2] = {&t29m_fwd_, &t29m_inv_};
    DeviceBuffer* bs[2] = {&t29s_fwd_, &t29s_inv_};
    const Fr* mont[2] = {twm_fwd_.as<Fr>(), twm_inv_.as<Fr>()};
    for (int dir = 0; dir < 2; ++dir) {
      auto* m29 = static_cast<fr29::TwMont29*>(bm[dir]->ensure(std::max<size_t>(1, split29_) * sizeof(fr29::TwMont29)));
      auto* s29 = static_cast<fr29::TwShoup29*>(bs[dir]->ensure(std::max<size_t>(1, nshoup) * sizeof(fr29::TwShoup29)));
      hipLaunchKernelGGL(tw29_table_kernel, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, stream_, m29, s29,
                         mont[dir], (uint32_t)split29_, (uint32_t)count);
    }
    TA_HIP(hipGetLastError());
    TA_HIP(hipStreamSynchronize(stream_));
  }
}

// The 32-bit Shoup tables {plain w, floor(w 2^256 / p)} of dif_pass_kernel's
// later passes (BN254 Fr under set_variant bit 0)
template <class Fr>
void NttDomain<Fr>::ensure_tables32() {
  using Tw = typename NttTw<Fr>::type;
  if constexpr (!std::is_same_v<Tw, Fr>) {
    if (tables32_ || log_n_ == 0) return;
    const uint32_t count = (uint32_t)(n_ - 1);
    Tw* tab[2] = {static_cast<Tw*>(tw_fwd_.ensure(n_ * sizeof(Tw))), static_cast<Tw*>(tw_inv_.ensure(n_ * sizeof(Tw)))};
    const Fr* mont[2] = {twm_fwd_.as<Fr>(), twm_inv_.as<Fr>()};
    for (int dir = 0; dir < 2; ++dir)
      hipLaunchKernelGGL(shoup_table_kernel<Fr>, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, stream_, tab[dir],
                         mont[dir], count);
    TA_HIP(hipGetLastError());
    TA_HIP(hipStreamSynchronize(stream_));
    tables32_ = true;
  }
}

template <class Fr>
bool NttDomain<Fr>::set_variant(int v) {
  if (v < 0 || v > 7 || (v & 3) == 2) return false;  // bit 1 (the LDS swizzle) modifies bit 0
  if ((v & 3) != 0 && !std::is_same_v<Fr, Bn254Fr>) return false;
  variant_ = v;
  if (v & 1) build_tables29();
  return true;
}

// Variant bit 2 turns the packing of one-pass transforms off (A/B)
template <class Fr>
uint32_t NttDomain<Fr>::pack_log(size_t batch) const {
  return (variant_ & 4) ? 0 : ntt::pack_log(plan_.size(), log_n_, batch);
}

template <class Fr>
typename NttDomain<Fr>::StageTables NttDomain<Fr>::stage_tables(bool inverse) const {
  const DeviceBuffer& tw = inverse ? tw_inv_ : tw_fwd_;
  const DeviceBuffer& twm = inverse ? twm_inv_ : twm_fwd_;
  return {tw.as<void>(), Tables32<Fr>::kShoup ? twm.as<Fr>() : tw.as<Fr>()};
}

template <class Fr>
size_t NttDomain<Fr>::stage_table_bytes() const {
  return tw_fwd_.capacity() + tw_inv_.capacity() + twm_fwd_.capacity() + twm_inv_.capacity();
}

template <class Fr>
void NttDomain<Fr>::build_powers(const Fr& base, const Fr& scale, Fr* d_lo, Fr* d_hi) {
  const size_t lo_cnt = size_t(1) << pow_bits_;
  const size_t hi_cnt = std::max<size_t>(1, n_ >> pow_bits_);
  std::vector<Fr> lo_h = host_powers(base, scale, lo_cnt);
  Fr step = base;
  for (uint32_t i = 0; i < pow_bits_; ++i) step = step.sqr();
  std::vector<Fr> hi_h = host_powers(step, Fr::one(), hi_cnt);
  TA_HIP(hipMemcpyAsync(d_lo, lo_h.data(), lo_cnt * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  TA_HIP(hipMemcpyAsync(d_hi, hi_h.data(), hi_cnt * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
}

template <class Fr>
void NttDomain<Fr>::set_offset(const Fr& h) {
  offset_ = h;
  has_offset_ = !h.is_one();
  offset_inv_ = has_offset_ ? h.inverse() : Fr::one();
  if (!has_offset_) return;
  const size_t lo_cnt = size_t(1) << pow_bits_;
  const size_t hi_cnt = std::max<size_t>(1, n_ >> pow_bits_);
  // forward: multiply input i by h^i ; inverse: output i by n^-1 h^-i
  build_powers(h, Fr::one(), static_cast<Fr*>(coset_lo_.ensure(lo_cnt * sizeof(Fr))),
               static_cast<Fr*>(coset_hi_.ensure(hi_cnt * sizeof(Fr))));
  build_powers(offset_inv_, size_inv_, static_cast<Fr*>(icoset_lo_.ensure(lo_cnt * sizeof(Fr))),
               static_cast<Fr*>(icoset_hi_.ensure(hi_cnt * sizeof(Fr))));
}

template <class Fr>
void NttDomain<Fr>::run(Fr* d_data, bool inverse, size_t batch, const Fr* src_in, const FourStepTw<Fr>* fs) {
  if (log_n_ == 0 || batch == 0) {
    // size-1 domain: forward is the identity (h^0 = 1); inverse scales by n^-1 = 1
    if (fs) throw std::runtime_error("tachyon_mi355x: four-step sub-transforms need >= 2 points");
    if (src_in && src_in != d_data && batch)
      TA_HIP(hipMemcpyAsync(d_data, src_in, batch * n_ * sizeof(Fr), hipMemcpyDeviceToDevice, stream_));
    return;
  }
  if (batch > 65535) throw std::runtime_error("tachyon_mi355x: NTT batch exceeds the grid limit");
  if (std::is_same_v<Fr, Bn254Fr> && (variant_ & 1)) {
    run29(d_data, inverse, batch, src_in, fs);
  } else {
    const StageTables st = stage_tables(inverse);
    const Tables32<Fr> tables{static_cast<const typename Tables32<Fr>::Tw*>(st.tw), st.twm, shoup_mode_, radix_,
                              ntt_variant_};
    void* scratch = plan_.size() > 1 ? scratch_.ensure(batch * n_ * sizeof(Fr)) : nullptr;
    const CosetPtrs<Fr> cp{coset_lo_.as<Fr>(), coset_hi_.as<Fr>(), icoset_lo_.as<Fr>(), icoset_hi_.as<Fr>()};
    run_passes(tables, plan_, log_n_, inverse, batch, pack_log(batch), size_inv_, has_offset_ ? &cp : nullptr, fs, src_in,
               d_data, scratch, stream_, profile_ ? ev_.data() : nullptr);
  }
  if (profile_) {
    TA_HIP(hipEventSynchronize(ev_[plan_.size()]));
    timings_.passes.assign(plan_.size(), 0.f);
    for (size_t p = 0; p < plan_.size(); ++p) TA_HIP(hipEventElapsedTime(&timings_.passes[p], ev_[p], ev_[p + 1]));
    TA_HIP(hipEventElapsedTime(&timings_.total, ev_[0], ev_[plan_.size()]));
  }
}

// BN254 Fr: the passes over 9 x 29-bit limbs (dif29_pass_kernel), called by run()
template <class Fr>
void NttDomain<Fr>::run29(Fr* d_data, bool inverse, size_t batch, const Fr* src_in, const FourStepTw<Fr>* fs) {
  if constexpr (std::is_same_v<Fr, Bn254Fr>) {
    const Tables29<Fr> tables{(inverse ? t29m_inv_ : t29m_fwd_).template as<fr29::TwMont29>(),
                              (inverse ? t29s_inv_ : t29s_fwd_).template as<fr29::TwShoup29>(), (uint32_t)split29_,
                              (variant_ & 2) != 0};
    void* scratch = plan_.size() > 1 ? scratch29_.ensure(batch * n_ * sizeof(F29)) : nullptr;
    const CosetPtrs<Fr> cp{coset_lo_.as<Fr>(), coset_hi_.as<Fr>(), icoset_lo_.as<Fr>(), icoset_hi_.as<Fr>()};
    run_passes(tables, plan_, log_n_, inverse, batch, pack_log(batch), size_inv_, has_offset_ ? &cp : nullptr, fs, src_in,
               d_data, scratch, stream_, profile_ ? ev_.data() : nullptr);
  }
}

template <class Fr>
void NttDomain<Fr>::forward_device(Fr* d_data, size_t batch) { run(d_data, false, batch); }

template <class Fr>
void NttDomain<Fr>::transform_device(const Fr* src, Fr* dst, bool inverse, size_t batch, const FourStepTw<Fr>* fs) {
  run(dst, inverse, batch, src, fs);
}

template <class Fr>
void NttDomain<Fr>::inverse_device(Fr* d_data, size_t batch) { run(d_data, true, batch); }

template <class Fr>
void NttDomain<Fr>::forward_host(const Fr* in, size_t len, Fr* out) {
  if (len > n_) throw std::runtime_error("tachyon_mi355x: FFT input longer than the domain");
  Fr* d = static_cast<Fr*>(io_.ensure(n_ * sizeof(Fr)));
  TA_HIP(hipMemcpyAsync(d, in, len * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  if (len < n_) TA_HIP(hipMemsetAsync(d + len, 0, (n_ - len) * sizeof(Fr), stream_));
  run(d, false, 1);
  TA_HIP(hipMemcpyAsync(out, d, n_ * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
}

template <class Fr>
void NttDomain<Fr>::inverse_host(const Fr* in, size_t len, Fr* out) {
  if (len > n_) throw std::runtime_error("tachyon_mi355x: IFFT input longer than the domain");
  Fr* d = static_cast<Fr*>(io_.ensure(n_ * sizeof(Fr)));
  TA_HIP(hipMemcpyAsync(d, in, len * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  if (len < n_) TA_HIP(hipMemsetAsync(d + len, 0, (n_ - len) * sizeof(Fr), stream_));
  run(d, true, 1);
  TA_HIP(hipMemcpyAsync(out, d, n_ * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
}

// ---------------------------------------------------------------------------
// NttGenDomain: one generator, every power-of-two size up to its order

template <class Fr>
NttGenDomain<Fr>::NttGenDomain(hipStream_t stream) : stream_(stream) {
  require_gpu();
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
}

template <class Fr>
NttGenDomain<Fr>::~NttGenDomain() {
  release();
  if (own_stream_) (void)hipStreamDestroy(stream_);
}

template <class Fr>
bool NttGenDomain<Fr>::init(const Fr& group_gen) {
  if (base_) return group_gen == gen_;
  // the order by repeated squaring: exactly 2^ln (0 never reaches 1, an
  // element of another order not within the field's two-adicity)
  constexpr uint32_t kMaxLog = std::min<uint32_t>((uint32_t)Fr::Config::kTwoAdicity, 30);
  uint32_t ln = 0;
  for (Fr x = group_gen; !x.is_one(); x = x.sqr(), ++ln)
    if (ln == kMaxLog) return false;
  base_.reset(new NttDomain<Fr>(group_gen, ln, stream_));
  log_n_ = ln;
  gen_ = group_gen.canonical();
  plans_.clear();
  size_inv_.clear();
  for (uint32_t L = 0; L <= ln; ++L) {
    plans_.push_back(pass_plan<Pass>(L, kMaxLdsElems, kMaxPassStages));
    size_inv_.push_back(fr_from_u64<Fr>(uint64_t(1) << L).inverse());
  }
  if constexpr (std::is_same_v<Fr, Bn254Fr>) {
    // both forms for the stage-table rows any L <= 20 reads on the 29-bit
    // passes: R'-form for the last min(N, 2^20) - 1 entries (rows >= LN - 20),
    // Shoup for the last min(N, 2^14) - 1 (rows >= LN - 14)
    const size_t n = size_t(1) << ln;
    cap29m_ = std::min<size_t>(n, size_t(1) << 20);
    cap29s_ = std::min<size_t>(n, size_t(1) << 14);
    DeviceBuffer* bm[2] = {&t29m_fwd_, &t29m_inv_};
    DeviceBuffer* bs[2] = {&t29s_fwd_, &t29s_inv_};
    const Fr* mont[2] = {base_->stage_tables(false).twm, base_->stage_tables(true).twm};
    for (int dir = 0; dir < 2 && n > 1; ++dir) {
      const uint32_t cm = (uint32_t)(cap29m_ - 1), cs = (uint32_t)(cap29s_ - 1);
      auto* m29 = static_cast<fr29::TwMont29*>(bm[dir]->ensure(cm * sizeof(fr29::TwMont29)));
      auto* s29 = static_cast<fr29::TwShoup29*>(bs[dir]->ensure(cs * sizeof(fr29::TwShoup29)));
      hipLaunchKernelGGL(tw29_table_kernel, dim3(ceil_div(cm, kBlock)), dim3(kBlock), 0, stream_, m29,
                         static_cast<fr29::TwShoup29*>(nullptr), mont[dir] + (n - cap29m_), cm, cm);
      hipLaunchKernelGGL(tw29_table_kernel, dim3(ceil_div(cs, kBlock)), dim3(kBlock), 0, stream_,
                         static_cast<fr29::TwMont29*>(nullptr), s29, mont[dir] + (n - cap29s_), 0u, cs);
    }
    TA_HIP(hipGetLastError());
  }
  TA_HIP(hipStreamSynchronize(stream_));
  return true;
}

template <class Fr>
void NttGenDomain<Fr>::release() {
  if (stream_) (void)hipStreamSynchronize(stream_);
  base_.reset();
  plans_.clear();
  size_inv_.clear();
  log_n_ = 0;
  cap29m_ = cap29s_ = 0;
  for (DeviceBuffer* b : {&t29m_fwd_, &t29m_inv_, &t29s_fwd_, &t29s_inv_, &scratch_, &io_}) b->release();
  for (CosetTables& c : cosets_) {
    c.used = 0;
    for (DeviceBuffer* b : {&c.lo, &c.hi, &c.ilo, &c.ihi}) b->release();
  }
}

template <class Fr>
size_t NttGenDomain<Fr>::table_bytes() const {
  if (!base_) return 0;
  size_t bytes = base_->stage_table_bytes() + t29m_fwd_.capacity() + t29m_inv_.capacity() + t29s_fwd_.capacity() +
                 t29s_inv_.capacity();
  for (const CosetTables& c : cosets_) bytes += c.lo.capacity() + c.hi.capacity() + c.ilo.capacity() + c.ihi.capacity();
  return bytes;
}

template <class Fr>
size_t NttGenDomain<Fr>::table_bytes_bound(uint32_t log_order) {
  const size_t n = size_t(1) << log_order, floor = 256;  // a DeviceBuffer's least allocation
  using Tw = typename NttTw<Fr>::type;
  // build_twiddles: the pass kernel's entries, and the Montgomery ones beside Shoup entries; both directions
  size_t bytes = 2 * (n * sizeof(Tw) + floor);
  if constexpr (!std::is_same_v<Tw, Fr>) bytes += 2 * (n * sizeof(Fr) + floor);
  if constexpr (std::is_same_v<Fr, Bn254Fr>)  // init: the 29-bit tables
    bytes += 2 * (std::min<size_t>(n, size_t(1) << 20) * sizeof(fr29::TwMont29) + floor) +
             2 * (std::min<size_t>(n, size_t(1) << 14) * sizeof(fr29::TwShoup29) + floor);
  // coset_tables: lo and hi of both directions per cached entry
  const size_t lo_max = size_t(1) << ((log_order + 1) / 2), hi_max = size_t(1) << (log_order / 2);
  return bytes + kCosetCacheEntries * 2 * ((lo_max + hi_max) * sizeof(Fr) + 2 * floor);
}

template <class Fr>
size_t NttGenDomain<Fr>::scratch_bytes_bound(uint32_t log_m, size_t batch) {
  // run29 / run32: one scratch array per batch entry when the plan has more than one pass
  const bool is29 = std::is_same_v<Fr, Bn254Fr> && log_m >= 1 && log_m <= 20;
  return std::max<size_t>(256, (batch << log_m) * (is29 ? sizeof(fr29::F29) : sizeof(Fr)));
}

// The power tables of (log_m, h): the cached entry, or the least recently
// used one rebuilt on the device.  An entry's buffers are allocated once, at
// the sizes of the largest sub-domain, so a rebuild only enqueues two kernels
// behind the passes that still read the old values.
template <class Fr>
const typename NttGenDomain<Fr>::CosetTables& NttGenDomain<Fr>::coset_tables(uint32_t log_m, const Fr& h) {
  CosetTables* victim = &cosets_[0];
  for (CosetTables& c : cosets_) {
    if (c.used && c.log_m == log_m && c.h == h) {
      c.used = ++tick_;
      return c;
    }
    if (c.used < victim->used) victim = &c;
  }
  CosetTables& c = *victim;
  const size_t lo_max = size_t(1) << ((log_n_ + 1) / 2), hi_max = size_t(1) << (log_n_ / 2);
  Fr* lo = static_cast<Fr*>(c.lo.ensure(lo_max * sizeof(Fr)));
  Fr* hi = static_cast<Fr*>(c.hi.ensure(hi_max * sizeof(Fr)));
  Fr* ilo = static_cast<Fr*>(c.ilo.ensure(lo_max * sizeof(Fr)));
  Fr* ihi = static_cast<Fr*>(c.ihi.ensure(hi_max * sizeof(Fr)));
  const uint32_t bits = (log_m + 1) / 2;
  const uint32_t lo_cnt = 1u << bits, hi_cnt = 1u << (log_m - bits);
  const unsigned blocks = ceil_div((size_t)lo_cnt + hi_cnt, kBlock);
  // forward: input i times h^i; inverse: output i times m^-1 h^-i
  hipLaunchKernelGGL(coset_powers_kernel<Fr>, dim3(blocks), dim3(kBlock), 0, stream_, lo, hi, h, Fr::one(), bits,
                     lo_cnt, hi_cnt);
  hipLaunchKernelGGL(coset_powers_kernel<Fr>, dim3(blocks), dim3(kBlock), 0, stream_, ilo, ihi, h.inverse(),
                     size_inv_[log_m], bits, lo_cnt, hi_cnt);
  TA_HIP(hipGetLastError());
  c.log_m = log_m;
  c.h = h;
  c.used = ++tick_;
  return c;
}

template <class Fr>
bool NttGenDomain<Fr>::uses29(uint32_t log_m) const {
  // NttDomain's default variant: BN254 Fr on the 29-bit passes up to 2^20
  return std::is_same_v<Fr, Bn254Fr> && log_m >= 1 && log_m <= 20;
}

template <class Fr>
void NttGenDomain<Fr>::run(Fr* d_data, uint32_t log_m, bool inverse, size_t batch, const Fr& coset) {
  if (!base_) throw std::runtime_error("tachyon_mi355x: NTT run before init");
  if (log_m > log_n_) throw std::runtime_error("tachyon_mi355x: NTT size above the initialised domain");
  // size 1: forward is the identity (h^0 = 1); inverse scales by 1^-1
  if (log_m == 0 || batch == 0) return;
  if (batch > 65535) throw std::runtime_error("tachyon_mi355x: NTT batch exceeds the grid limit");
  const CosetTables* ct = coset.is_one() ? nullptr : &coset_tables(log_m, coset);
  if (uses29(log_m)) run29(d_data, log_m, inverse, batch, ct);
  else run32(d_data, log_m, inverse, batch, ct);
}

template <class Fr>
void NttGenDomain<Fr>::run_host(Fr* data, uint32_t log_m, bool inverse, size_t batch, const Fr& coset) {
  const size_t bytes = (batch << log_m) * sizeof(Fr);
  Fr* d = static_cast<Fr*>(io_.ensure(bytes));
  TA_HIP(hipMemcpyAsync(d, data, bytes, hipMemcpyHostToDevice, stream_));
  run(d, log_m, inverse, batch, coset);
  TA_HIP(hipMemcpyAsync(data, d, bytes, hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
}

// The 32-bit passes on the size-N tables' suffix: the table bases advanced by
// N - m, PassArgs::L = log_m
template <class Fr>
void NttGenDomain<Fr>::run32(Fr* d_data, uint32_t log_m, bool inverse, size_t batch, const CosetTables* ct) {
  const size_t m = size_t(1) << log_m, shift = (size_t(1) << log_n_) - m;
  const auto st = base_->stage_tables(inverse);
  const Tables32<Fr> tables{static_cast<const typename Tables32<Fr>::Tw*>(st.tw) + shift, st.twm + shift};
  const std::vector<Pass>& plan = plans_[log_m];
  void* scratch = plan.size() > 1 ? scratch_.ensure(batch * m * sizeof(Fr)) : nullptr;
  CosetPtrs<Fr> cp{};
  if (ct) cp = {ct->lo.template as<Fr>(), ct->hi.template as<Fr>(), ct->ilo.template as<Fr>(), ct->ihi.template as<Fr>()};
  run_passes<Fr>(tables, plan, log_m, inverse, batch, pack_log(plan.size(), log_m, batch), size_inv_[log_m],
                 ct ? &cp : nullptr, nullptr, nullptr, d_data, scratch, stream_, nullptr);
}

// The 29-bit passes (BN254 Fr, log_m <= 20) on the bounded 29-bit tables:
// entry (stage s, index j) of the size-m network is entry (m - (m >> s)) + j +
// (cap - m) of a table holding the last cap - 1 entries
template <class Fr>
void NttGenDomain<Fr>::run29(Fr* d_data, uint32_t log_m, bool inverse, size_t batch, const CosetTables* ct) {
  if constexpr (std::is_same_v<Fr, Bn254Fr>) {
    const size_t m = size_t(1) << log_m;
    Tables29<Fr> tables{(inverse ? t29m_inv_ : t29m_fwd_).template as<fr29::TwMont29>() + (cap29m_ - m),
                        (inverse ? t29s_inv_ : t29s_fwd_).template as<fr29::TwShoup29>(), 0u, false};
    if (m <= cap29s_) tables.ts += cap29s_ - m;
    else tables.ts_off = (uint32_t)(m - cap29s_);  // (later passes read stages >= k0 only: m >> k0 <= 2^14)
    const std::vector<Pass>& plan = plans_[log_m];
    void* scratch = plan.size() > 1 ? scratch_.ensure(batch * m * sizeof(F29)) : nullptr;
    CosetPtrs<Fr> cp{};
    if (ct) cp = {ct->lo.template as<Fr>(), ct->hi.template as<Fr>(), ct->ilo.template as<Fr>(), ct->ihi.template as<Fr>()};
    run_passes<Fr>(tables, plan, log_m, inverse, batch, pack_log(plan.size(), log_m, batch), size_inv_[log_m],
                   ct ? &cp : nullptr, nullptr, nullptr, d_data, scratch, stream_, nullptr);
  }
}

template <class Fr>
Ntt4Step<Fr>::Ntt4Step(uint32_t log_n, uint32_t log_world, uint32_t rank, hipStream_t stream, uint32_t log_r)
    : log_n_(log_n), log_g_(log_world), rank_(rank), n_(size_t(1) << log_n), stream_(stream) {
  require_gpu();
  log_r_ = log_r ? log_r : log_n / 2;
  if (log_r_ >= log_n) throw std::runtime_error("tachyon_mi355x: four-step NTT needs 1 <= log R < log n");
  log_c_ = log_n - log_r_;
  if (log_g_ > log_r_ || log_g_ > log_c_ || rank >= (1u << log_g_) || log_n > (uint32_t)Fr::Config::kTwoAdicity ||
      log_n > 30)
    throw std::runtime_error("tachyon_mi355x: four-step NTT needs R, C >= world size");
  if (!stream_) {
    TA_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
  dom_r_ = new NttDomain<Fr>(size_t(1) << log_r_, stream_);
  dom_c_ = new NttDomain<Fr>(size_t(1) << log_c_, stream_);
  // w_n and its two-level power tables (w_n^e = lo[e & mask] * hi[e >> bits])
  Fr w = two_adic_root<Fr>();
  for (uint32_t i = log_n; i < (uint32_t)Fr::Config::kTwoAdicity; ++i) w = w.sqr();
  w_ = w;
  pow_bits_ = (log_n + 1) / 2;
  const size_t lo_cnt = size_t(1) << pow_bits_, hi_cnt = size_t(1) << (log_n - pow_bits_);
  const Fr wi = w.inverse();
  DeviceBuffer* bufs[4] = {&w_lo_, &w_hi_, &wi_lo_, &wi_hi_};
  const Fr bases[2] = {w, wi};
  for (int d = 0; d < 2; ++d) {
    Fr step = bases[d];
    for (uint32_t i = 0; i < pow_bits_; ++i) step = step.sqr();
    std::vector<Fr> lo_h = host_powers(bases[d], Fr::one(), lo_cnt);
    std::vector<Fr> hi_h = host_powers(step, Fr::one(), hi_cnt);
    TA_HIP(hipMemcpyAsync(bufs[2 * d]->ensure(lo_cnt * sizeof(Fr)), lo_h.data(), lo_cnt * sizeof(Fr),
                          hipMemcpyHostToDevice, stream_));
    TA_HIP(hipMemcpyAsync(bufs[2 * d + 1]->ensure(hi_cnt * sizeof(Fr)), hi_h.data(), hi_cnt * sizeof(Fr),
                          hipMemcpyHostToDevice, stream_));
    TA_HIP(hipStreamSynchronize(stream_));
  }
}

template <class Fr>
Ntt4Step<Fr>::~Ntt4Step() {
  delete dom_r_;
  delete dom_c_;
  if (own_stream_) (void)hipStreamDestroy(stream_);
}

// Stage 1 forward: the R-point NTTs of the local columns read `in` directly
// (no copy) and their last pass multiplies by w_n^(c k1) and writes the packed
// send layout (no separate twiddle kernel): two HBM round trips for R <= 2^16.
// (Before round 5: a copy, the passes, and twiddle_exchange_kernel -- kept as
// the unfused path, fused_ = false, for A/B.)
// The exchange twiddles of one direction as FourStepTw::tab29, built on first
// use when the column NTTs run on the 29-bit passes (nullptr otherwise: the
// 32-bit passes compute them)
template <class Fr>
const void* Ntt4Step<Fr>::exchange_table(bool inverse) {
  if constexpr (!std::is_same_v<Fr, Bn254Fr>) {
    (void)inverse;
    return nullptr;
  } else {
    if (!(dom_r_->variant() & 1) || no_table_) return nullptr;
    DeviceBuffer& t = inverse ? tab29_inv_ : tab29_fwd_;
    if (!t.capacity()) {
      const uint32_t log_cg = log_c_ - log_g_, log_rg = log_r_ - log_g_;
      const FourStepTw<Fr> f{inverse ? wi_lo_.as<Fr>() : w_lo_.as<Fr>(), inverse ? wi_hi_.as<Fr>() : w_hi_.as<Fr>(),
                             pow_bits_, log_n_, log_rg, log_cg, rank_ << log_cg};
      const size_t count = local_size();
      auto* out = static_cast<fr29::TwMont29*>(t.ensure(count * sizeof(fr29::TwMont29)));
      hipLaunchKernelGGL(fs_table29_kernel, dim3(ceil_div(count, kBlock)), dim3(kBlock), 0, stream_, f, log_r_, count,
                         out);
      TA_HIP(hipGetLastError());
    }
    return t.as<void>();
  }
}

template <class Fr>
void Ntt4Step<Fr>::forward_stage1(const Fr* in, Fr* send) {
  const size_t m = local_size();
  const uint32_t log_cg = log_c_ - log_g_, log_rg = log_r_ - log_g_;
  if (fused_) {
    FourStepTw<Fr> fs{w_lo_.as<Fr>(), w_hi_.as<Fr>(), pow_bits_, log_n_, log_rg, log_cg, rank_ << log_cg};
    fs.tab29 = exchange_table(false);
    fs.log_r = log_r_;
    dom_r_->transform_device(in, send, false, size_t(1) << log_cg, &fs);
    return;
  }
  Fr* work = static_cast<Fr*>(work_.ensure(m * sizeof(Fr)));
  TA_HIP(hipMemcpyAsync(work, in, m * sizeof(Fr), hipMemcpyDeviceToDevice, stream_));
  dom_r_->forward_device(work, size_t(1) << log_cg);
  hipLaunchKernelGGL(twiddle_exchange_kernel<Fr>, dim3(ceil_div(m, kBlock)), dim3(kBlock), 0, stream_, work, send,
                     log_r_, log_rg, log_cg, rank_ << log_cg, log_n_, w_lo_.as<Fr>(), w_hi_.as<Fr>(), pow_bits_, 0u);
  TA_HIP(hipGetLastError());
}

template <class Fr>
void Ntt4Step<Fr>::forward_stage2(const Fr* recv, Fr* out) {
  const uint32_t log_cg = log_c_ - log_g_, log_rg = log_r_ - log_g_;
  if (fused_) {
    // recv = G chunks [k1_l][c_l] (fs_packed): the C-point NTTs' first pass
    // reads each local row k1_l as G runs of Cg elements (kLoadXch) -- no
    // transpose.  A one-pass C NTT in place would read what other workgroups
    // write: recv goes through the work buffer then.
    FourStepTw<Fr> fs{};
    fs.log_rg = log_rg;
    fs.log_cg = log_cg;
    fs.rows = 1;
    const Fr* src = recv;
    if (recv == out && dom_c_->plan().size() == 1) {
      Fr* work = static_cast<Fr*>(work_.ensure(local_size() * sizeof(Fr)));
      TA_HIP(hipMemcpyAsync(work, recv, local_size() * sizeof(Fr), hipMemcpyDeviceToDevice, stream_));
      src = work;
    }
    dom_c_->transform_device(src, out, false, size_t(1) << log_rg, &fs);
    return;
  }
  // round 4: recv = [c][k1_l] (C x Rg) -> out = [k1_l][c], then C-point NTTs on the rows
  const uint32_t rows = 1u << log_c_, cols = 1u << log_rg;
  hipLaunchKernelGGL(transpose_kernel<Fr>, dim3(ceil_div(cols, 32), ceil_div(rows, 32)), dim3(kBlock), 0, stream_,
                     recv, out, rows, cols);
  TA_HIP(hipGetLastError());
  dom_c_->forward_device(out, cols);
}

template <class Fr>
void Ntt4Step<Fr>::inverse_stage1(const Fr* in, Fr* send) {
  // in = [k1_l][k2] (Rg x C): inverse C-point NTTs on the rows
  const size_t m = local_size();
  const uint32_t log_cg = log_c_ - log_g_, log_rg = log_r_ - log_g_;
  const uint32_t rows = 1u << log_rg, cols = 1u << log_c_;
  if (fused_) {
    // the last pass writes the exchange layout, G chunks [k1_l][c_l]
    // (kStoreXch) -- no transpose; in place (in == send) through the work buffer
    FourStepTw<Fr> fs{};
    fs.log_rg = log_rg;
    fs.log_cg = log_cg;
    fs.rows = 1;
    if (in == send) {
      Fr* work = static_cast<Fr*>(work_.ensure(m * sizeof(Fr)));
      dom_c_->transform_device(in, work, true, rows, &fs);
      TA_HIP(hipMemcpyAsync(send, work, m * sizeof(Fr), hipMemcpyDeviceToDevice, stream_));
    } else {
      dom_c_->transform_device(in, send, true, rows, &fs);
    }
    return;
  }
  // round 4: a copy, the inverse passes, then the transpose to [c][k1_l] = G chunks [c_l][k1_l]
  Fr* work = static_cast<Fr*>(work_.ensure(m * sizeof(Fr)));
  TA_HIP(hipMemcpyAsync(work, in, m * sizeof(Fr), hipMemcpyDeviceToDevice, stream_));
  dom_c_->inverse_device(work, rows);
  hipLaunchKernelGGL(transpose_kernel<Fr>, dim3(ceil_div(cols, 32), ceil_div(rows, 32)), dim3(kBlock), 0, stream_,
                     work, send, rows, cols);
  TA_HIP(hipGetLastError());
}

template <class Fr>
void Ntt4Step<Fr>::inverse_stage2(const Fr* recv, Fr* out) {
  const size_t m = local_size();
  const uint32_t log_cg = log_c_ - log_g_, log_rg = log_r_ - log_g_;
  if (fused_) {  // the unpack and w_n^-(c k1) in the first pass's load
    FourStepTw<Fr> fs{wi_lo_.as<Fr>(), wi_hi_.as<Fr>(), pow_bits_, log_n_, log_rg, log_cg, rank_ << log_cg};
    fs.tab29 = exchange_table(true);
    fs.log_r = log_r_;
    dom_r_->transform_device(recv, out, true, size_t(1) << log_cg, &fs);
    return;
  }
  hipLaunchKernelGGL(twiddle_exchange_kernel<Fr>, dim3(ceil_div(m, kBlock)), dim3(kBlock), 0, stream_, recv, out,
                     log_r_, log_rg, log_cg, rank_ << log_cg, log_n_, wi_lo_.as<Fr>(), wi_hi_.as<Fr>(), pow_bits_, 1u);
  TA_HIP(hipGetLastError());
  dom_r_->inverse_device(out, size_t(1) << log_cg);
}

template <class Fr>
NttMultiDevice<Fr>::NttMultiDevice(uint32_t log_n, const std::vector<int>& devices, int primary,
                                   hipStream_t primary_stream)
    : log_n_(log_n), n_(size_t(1) << log_n), primary_(primary), s0_(primary_stream), ids_(devices) {
  const size_t G = devices.size();
  if (G < 2 || (G & (G - 1))) throw std::runtime_error("tachyon_mi355x: multi-device NTT needs 2^k >= 2 devices");
  log_g_ = (uint32_t)__builtin_ctzll(G);
  log_r_ = ntt4_split_log_r(log_n, log_g_);  // the fewest pass launches (2^24: 2^8 x 2^16)
  log_c_ = log_n - log_r_;
  if (log_g_ > log_r_ || log_g_ > log_c_)
    throw std::runtime_error("tachyon_mi355x: multi-device NTT needs R, C >= devices");
  int count = 0, prev = 0;
  TA_HIP(hipGetDeviceCount(&count));
  for (int d : devices)
    if (d < 0 || d >= count) throw std::runtime_error("tachyon_mi355x: device id out of range");
  TA_HIP(hipGetDevice(&prev));
  struct Restore {
    int d;
    ~Restore() { (void)hipSetDevice(d); }
  } restore{prev};
  TA_HIP(hipSetDevice(primary_));
  TA_HIP(hipEventCreateWithFlags(&ev0_, hipEventDisableTiming));
  for (int d : devices)  // xGMI peer access where the pair supports it (copies work without it)
    if (d != primary_) {
      int ok = 0;
      if (hipDeviceCanAccessPeer(&ok, primary_, d) == hipSuccess && ok) (void)hipDeviceEnablePeerAccess(d, 0);
      (void)hipGetLastError();
    }
  for (size_t g = 0; g < G; ++g) {
    TA_HIP(hipSetDevice(devices[g]));
    auto p = std::make_unique<Part>();
    p->device = devices[g];
    TA_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    TA_HIP(hipEventCreateWithFlags(&p->ev1, hipEventDisableTiming));
    TA_HIP(hipEventCreateWithFlags(&p->ev2, hipEventDisableTiming));
    p->plan = std::make_unique<Ntt4Step<Fr>>(log_n, log_g_, (uint32_t)g, p->stream, log_r_);
    const size_t m = n_ >> log_g_;
    p->in.ensure(m * sizeof(Fr));
    p->send.ensure(m * sizeof(Fr));
    p->recv.ensure(m * sizeof(Fr));
    p->out.ensure(m * sizeof(Fr));
    for (int e : devices)
      if (e != devices[g]) {
        int ok = 0;
        if (hipDeviceCanAccessPeer(&ok, devices[g], e) == hipSuccess && ok) (void)hipDeviceEnablePeerAccess(e, 0);
        (void)hipGetLastError();
      }
    parts_.push_back(std::move(p));
  }
  TA_HIP(hipSetDevice(primary_));
  stage_.ensure(n_ * sizeof(Fr));
}

template <class Fr>
NttMultiDevice<Fr>::~NttMultiDevice() {
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess) prev = 0;
  for (auto& p : parts_) {  // each part's stream, events and buffers on its own device
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);
    p->plan.reset();
    p->in.release();
    p->send.release();
    p->recv.release();
    p->out.release();
    (void)hipEventDestroy(p->ev1);
    (void)hipEventDestroy(p->ev2);
    (void)hipStreamDestroy(p->stream);
  }
  (void)hipSetDevice(primary_);
  (void)hipStreamSynchronize(s0_);
  stage_.release();
  io_.release();
  if (ev0_) (void)hipEventDestroy(ev0_);
  (void)hipSetDevice(prev);
}

// forward: stage = x^T (x as R x C), part g's input = stage chunk g (its
//   columns, column-major); stage 1; all-to-all; stage 2 -> rows [g R/G,
//   (g+1) R/G) of Z[k1][k2] = X[k1 + R k2]; the parts' rows = Z (R x C) in
//   stage; y = Z^T.  Both transposes take an R x C matrix.
// inverse: stage = Z = y^T (y as C x R), part g's input = rows chunk g;
//   inverse stages 1, 2 -> columns; the parts' columns = x^T (C x R); x = its
//   transpose.  Both transposes take a C x R matrix.
template <class Fr>
void NttMultiDevice<Fr>::run(const Fr* x, Fr* y, bool inverse) {
  const size_t G = parts_.size(), m = n_ >> log_g_, chunk = m >> log_g_;
  const uint32_t R = 1u << log_r_, C = 1u << log_c_;
  const uint32_t rows_in = inverse ? C : R, cols_in = inverse ? R : C;
  int prev = 0;
  TA_HIP(hipGetDevice(&prev));
  struct Restore {
    int d;
    ~Restore() { (void)hipSetDevice(d); }
  } restore{prev};
  TA_HIP(hipSetDevice(primary_));
  Fr* stage = stage_.as<Fr>();
  hipLaunchKernelGGL(transpose_kernel<Fr>, dim3(ceil_div(cols_in, 32), ceil_div(rows_in, 32)), dim3(kBlock), 0, s0_,
                     x, stage, rows_in, cols_in);
  TA_HIP(hipGetLastError());
  TA_HIP(hipEventRecord(ev0_, s0_));
  for (size_t g = 0; g < G; ++g) {  // scatter + stage 1
    Part& p = *parts_[g];
    TA_HIP(hipSetDevice(p.device));
    TA_HIP(hipStreamWaitEvent(p.stream, ev0_, 0));
    TA_HIP(hipMemcpyPeerAsync(p.in.template as<void>(), p.device, stage + g * m, primary_, m * sizeof(Fr), p.stream));
    if (inverse) p.plan->inverse_stage1(p.in.template as<Fr>(), p.send.template as<Fr>());
    else p.plan->forward_stage1(p.in.template as<Fr>(), p.send.template as<Fr>());
    TA_HIP(hipEventRecord(p.ev1, p.stream));
  }
  for (size_t h = 0; h < G; ++h) {  // all-to-all: chunk h of every part's send -> part h's recv + stage 2
    Part& q = *parts_[h];
    TA_HIP(hipSetDevice(q.device));
    for (size_t g = 0; g < G; ++g) TA_HIP(hipStreamWaitEvent(q.stream, parts_[g]->ev1, 0));
    for (size_t g = 0; g < G; ++g)
      TA_HIP(hipMemcpyPeerAsync(q.recv.template as<Fr>() + g * chunk, q.device, parts_[g]->send.template as<Fr>() + h * chunk,
                                parts_[g]->device, chunk * sizeof(Fr), q.stream));
    if (inverse) q.plan->inverse_stage2(q.recv.template as<Fr>(), q.out.template as<Fr>());
    else q.plan->forward_stage2(q.recv.template as<Fr>(), q.out.template as<Fr>());
    TA_HIP(hipEventRecord(q.ev2, q.stream));
  }
  TA_HIP(hipSetDevice(primary_));
  for (size_t g = 0; g < G; ++g) {  // gather on the primary stream
    Part& p = *parts_[g];
    TA_HIP(hipStreamWaitEvent(s0_, p.ev2, 0));
    TA_HIP(hipMemcpyPeerAsync(stage + g * m, primary_, p.out.template as<void>(), p.device, m * sizeof(Fr), s0_));
  }
  hipLaunchKernelGGL(transpose_kernel<Fr>, dim3(ceil_div(cols_in, 32), ceil_div(rows_in, 32)), dim3(kBlock), 0, s0_,
                     stage, y, rows_in, cols_in);
  TA_HIP(hipGetLastError());
}

template <class Fr>
void NttMultiDevice<Fr>::host(const Fr* in, size_t len, Fr* out, bool inverse) {
  if (len > n_) throw std::runtime_error("tachyon_mi355x: more inputs than the domain size");
  int prev = 0;
  TA_HIP(hipGetDevice(&prev));
  struct Restore {
    int d;
    ~Restore() { (void)hipSetDevice(d); }
  } restore{prev};
  TA_HIP(hipSetDevice(primary_));
  Fr* d = static_cast<Fr*>(io_.ensure(n_ * sizeof(Fr)));
  TA_HIP(hipMemcpyAsync(d, in, len * sizeof(Fr), hipMemcpyHostToDevice, s0_));
  if (len < n_) TA_HIP(hipMemsetAsync(d + len, 0, (n_ - len) * sizeof(Fr), s0_));
  run(d, d, inverse);
  TA_HIP(hipMemcpyAsync(out, d, n_ * sizeof(Fr), hipMemcpyDeviceToHost, s0_));
  TA_HIP(hipStreamSynchronize(s0_));
}

template <class Fr>
Fr root_of_unity(uint32_t log_n) {
  if (log_n > (uint32_t)Fr::Config::kTwoAdicity)
    throw std::runtime_error("tachyon_mi355x: no root of unity of that order in the field");
  Fr w = two_adic_root<Fr>();
  for (uint32_t i = log_n; i < (uint32_t)Fr::Config::kTwoAdicity; ++i) w = w.sqr();
  return w;
}
bool set_bn254_fr_halo2_generator(bool on) { return g_bn254_fr_halo2.exchange(on); }
bool bn254_fr_halo2_generator() { return g_bn254_fr_halo2.load(); }

template <class Fr>
Fr field_from_u64(uint64_t v) {
  return fr_from_u64<Fr>(v);
}

template class NttDomain<Bn254Fr>;
template class NttDomain<Bls381Fr>;
template class NttGenDomain<Bn254Fr>;
template class NttGenDomain<Bls381Fr>;
template Bn254Fr root_of_unity<Bn254Fr>(uint32_t);
template Bls381Fr root_of_unity<Bls381Fr>(uint32_t);
template Bn254Fr field_from_u64<Bn254Fr>(uint64_t);
template Bls381Fr field_from_u64<Bls381Fr>(uint64_t);
template class Ntt4Step<Bn254Fr>;

uint32_t ntt4_split_log_r(uint32_t log_n, uint32_t log_world) {
  auto passes = [](uint32_t k) { return (k + kMaxPassStages - 1) / kMaxPassStages; };
  uint32_t best = 0, best_cost = ~0u;
  for (uint32_t r = std::max(1u, log_world); r < log_n; ++r) {
    const uint32_t c = log_n - r;
    if (c < log_world || r > c) continue;
    const uint32_t cost = passes(r) + passes(c);
    if (cost <= best_cost) {  // ties: the larger R (up to C)
      best_cost = cost;
      best = r;
    }
  }
  return best ? best : log_n / 2;
}
template class NttMultiDevice<Bn254Fr>;

}  // namespace tachyon_amd::ntt
