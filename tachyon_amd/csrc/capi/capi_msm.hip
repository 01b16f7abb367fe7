// C-ABI of the MSM (include/tachyon_mi355x.h): the reference entry points per
// curve and the curve-generic tachyon_mi355x_msm_* extensions.
//
// Reference entry points restated here:
//   tachyon/c/math/elliptic_curves/generator/msm.cc.tpl, msm_gpu.cc.tpl
//   tachyon/c/math/elliptic_curves/msm/msm.h:13-48 (MSMApi / DoMSM)
//   tachyon/c/math/elliptic_curves/msm/msm_gpu.h:23-122 (MSMGpuApi / DoMSMGpu,
//     TACHYON_MSM_GPU_INPUT_DIR / TACHYON_LOG_MSM hooks)
#include "../../../include/tachyon_mi355x.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../dist/comm.h"
#include "../msm/msm.h"
#include "../msm/msm_multi.h"
#include "capi_guard.h"

using namespace tachyon_amd;

namespace {

template <class Curve>
struct MsmCtx {
  msm::MsmGpu<Curve> impl;
  // several devices (tachyon_mi355x_msm_gpu_set_devices or TACHYON_MSM_GPU_DEVICES): one point
  // shard per device, results added on the host (msm/msm_multi.h); null = impl on the current device
  std::unique_ptr<msm::MsmMultiDevice<Curve>> multi;
  std::string input_dir;  // TACHYON_MSM_GPU_INPUT_DIR
  bool log = false;       // TACHYON_LOG_MSM=1
  size_t idx = 0;
  explicit MsmCtx(hipStream_t stream = nullptr) : impl(stream) {
    if (const char* d = getenv("TACHYON_MSM_GPU_INPUT_DIR")) input_dir = d;
    if (const char* l = getenv("TACHYON_LOG_MSM")) log = (std::string(l) == "1");
    if (const char* e = getenv("TACHYON_MSM_GPU_DEVICES")) {
      const std::vector<int> ids = msm::parse_device_list(e);
      if (ids.empty()) throw std::runtime_error(std::string("TACHYON_MSM_GPU_DEVICES: malformed device list '") + e + "'");
      if (ids.size() > 1) multi = std::make_unique<msm::MsmMultiDevice<Curve>>(ids);
    }
  }
  XYZZ<typename Curve::F> run(const void* bases, const void* scalars, size_t n) {
    return multi ? multi->run(bases, scalars, n) : impl.run(bases, scalars, n);
  }
  // the engine whose timings, schedule and sizes stand for the last run
  // (multi-device: the shard that ran the most points)
  const msm::MsmGpu<Curve>& lead() const { return multi ? multi->lead() : impl; }
  // a setting goes to impl and, when present, to every shard of multi
  template <class Fn>
  void set(Fn&& setter) {
    setter(impl);
    if (multi) setter(*multi);
  }
};

template <class F>
void write_canonical(FILE* f, const F& x);

template <class C>
void write_canonical(FILE* f, const Fp<C>& x) {
  Fp<C> c = x.from_mont();
  fwrite(c.v, sizeof(c.v), 1, f);
}
template <class B>
void write_canonical(FILE* f, const Fp2<B>& x) {
  write_canonical(f, x.c0);
  write_canonical(f, x.c1);
}

// Replay dump (msm_gpu.h:99-119): u64 count, then canonical LE limbs
// (Buffer serialisation with s_is_in_montgomery = false, copyable.h:137-155).
template <class Curve>
void dump_inputs(const std::string& dir, size_t idx, const void* bases, const void* scalars, size_t n) {
  using F = typename Curve::F;
  using Fr = typename Curve::Fr;
  std::vector<Affine<F>> hb(n);
  std::vector<Fr> hs(n);
  TA_HIP(hipMemcpy(hb.data(), bases, n * sizeof(Affine<F>), hipMemcpyDefault));
  TA_HIP(hipMemcpy(hs.data(), scalars, n * sizeof(Fr), hipMemcpyDefault));
  std::string pb = dir + "/bases" + std::to_string(idx) + ".txt";
  std::string ps = dir + "/scalars" + std::to_string(idx) + ".txt";
  FILE* f = fopen(pb.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open " + pb);
  uint64_t cnt = n;
  fwrite(&cnt, 8, 1, f);
  for (auto& p : hb) {
    write_canonical(f, p.x);
    write_canonical(f, p.y);
  }
  fclose(f);
  f = fopen(ps.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open " + ps);
  fwrite(&cnt, 8, 1, f);
  for (auto& s : hs) write_canonical(f, s);
  fclose(f);
}

// canonical value in hex, "0x" + lowercase digits without leading zeros
// (BigInt::ToHexString, big_int.cc:55-58; fields print their canonical value)
template <class C>
void print_hex(const Fp<C>& x) {
  const Fp<C> c = x.from_mont();
  const uint32_t* l = c.v;
  int i = Fp<C>::N - 1;
  while (i > 0 && l[i] == 0) --i;
  printf("0x%x", l[i]);
  while (--i >= 0) printf("%08x", l[i]);
}
template <class B>
void print_hex(const Fp2<B>& x) {
  printf("(");
  print_hex(x.c0);
  printf(", ");
  print_hex(x.c1);
  printf(")");
}

// DoMSMGpu: run, normalise, return a new Jacobian (z = 1, or the (1,1,0) zero).
template <class Curve, class CJac>
CJac* do_msm(MsmCtx<Curve>* ctx, const void* bases, const void* scalars, size_t n) {
  using F = typename Curve::F;
  XYZZ<F> r = ctx->run(bases, scalars, n);
  Affine<F> a = r.to_affine();
  Jacobian<F> j = a.is_zero() ? Jacobian<F>::zero() : Jacobian<F>{a.x, a.y, F::one()};
  static_assert(sizeof(CJac) == sizeof(Jacobian<F>), "layout");
  CJac* out = new CJac();
  memcpy(out, &j, sizeof(j));
  if (ctx->log) {
    printf("DoMSMGpu()%zu\n(", ctx->idx);
    print_hex(a.x);
    printf(", ");
    print_hex(a.y);
    printf(")\n");
  }
  ctx->idx++;
  if (!ctx->input_dir.empty()) dump_inputs<Curve>(ctx->input_dir, ctx->idx - 1, bases, scalars, n);
  return out;
}

template <class Curve>
void msm_affine_out(void* ctx, const void* bases, const void* scalars, size_t n, void* out) {
  using F = typename Curve::F;
  auto* c = static_cast<MsmCtx<Curve>*>(ctx);
  Affine<F> a = c->run(bases, scalars, n).to_affine();
  memcpy(out, &a, sizeof(a));
}

template <class Curve>
void msm_window_range_out(void* ctx, const void* bases, const void* scalars, size_t n, unsigned w_begin,
                          unsigned w_end, void* out) {
  using F = typename Curve::F;
  auto* c = static_cast<MsmCtx<Curve>*>(ctx);
  Affine<F> a = c->impl.run_window_range(bases, scalars, n, w_begin, w_end).to_affine();
  memcpy(out, &a, sizeof(a));
}

template <class Curve>
void msm_folded_out(void* ctx, const void* folded_bases, const void* scalars, size_t n, unsigned fold, void* out) {
  using F = typename Curve::F;
  auto* c = static_cast<MsmCtx<Curve>*>(ctx);
  Affine<F> a = c->impl.run_folded(folded_bases, scalars, n, fold).to_affine();
  memcpy(out, &a, sizeof(a));
}

// `count` MSMs over the same device-resident bases in one launch sequence
// (MsmGpu::run_batch): count affine results ((0, 0) = identity)
template <class Curve>
void msm_batch_out(void* ctx, const void* bases, size_t len, const void* scalars, size_t count, void* out) {
  using F = typename Curve::F;
  auto* c = static_cast<MsmCtx<Curve>*>(ctx);
  const auto pts = c->impl.run_batch(bases, scalars, len, count);
  auto* o = static_cast<Affine<F>*>(out);
  for (size_t g = 0; g < count; ++g) o[g] = pts[g].to_affine();
}

// The MSM in the point form a C++ caller asks for (include/tachyon_mi355x_msm.h):
// 0 affine {x, y} ((0, 0) = identity); 1 projective / 2 Jacobian {x, y, z}
// (identity (1, 1, 0), projective_point.h:34-36, jacobian_point.h; otherwise
// z = 1); 3 XYZZ {x, y, zz, zzz} (identity (1, 1, 0, 0), point_xyzz.h:37-39) --
// the Bucket of VariableBaseMSM<AffinePoint> (pippenger_base.h:24-28).
template <class Curve>
void msm_form_out(void* ctx, const void* bases, const void* scalars, size_t n, int form, void* out) {
  using F = typename Curve::F;
  auto* c = static_cast<MsmCtx<Curve>*>(ctx);
  const Affine<F> a = c->run(bases, scalars, n).to_affine();
  switch (form) {
    case 0:
      memcpy(out, &a, sizeof(a));
      break;
    case 1:
    case 2: {
      const Jacobian<F> j = a.is_zero() ? Jacobian<F>::zero() : Jacobian<F>{a.x, a.y, F::one()};
      memcpy(out, &j, sizeof(j));
      break;
    }
    case 3: {
      const XYZZ<F> p = XYZZ<F>::from_affine(a);
      memcpy(out, &p, sizeof(p));
      break;
    }
    default:
      throw std::runtime_error("point form must be 0 (affine), 1 (projective), 2 (jacobian) or 3 (xyzz)");
  }
}

// Non-affine bases (VariableBaseMSM<ProjectivePoint / JacobianPoint /
// PointXYZZ>): normalised to affine on the device, then the MSM above
template <class Curve>
void msm_points_form_out(void* ctx, const void* bases, int base_form, const void* scalars, size_t n, int form,
                         void* out) {
  auto* c = static_cast<MsmCtx<Curve>*>(ctx);
  const void* aff = c->impl.affine_bases(bases, n, base_form);
  msm_form_out<Curve>(ctx, aff, scalars, n, form, out);
}

// One rank's shard of an MSM over a communicator: the local XYZZ partial,
// one all-gather of every rank's partial, the group sum in rank order (the
// same point on every rank) -- the kParallelTerm chunk-and-sum
// (pippenger_adapter.h:82-113) across processes, with the exchange inside
// the library (tachyon_amd.dist.sharded_msm is the torch.distributed form)
template <class Curve>
void msm_sharded_out(void* ctx, dist::Comm* comm, const void* bases, const void* scalars, size_t n, void* out) {
  using F = typename Curve::F;
  auto* c = static_cast<MsmCtx<Curve>*>(ctx);
  // (a rank whose local MSM fails still enters the exchange: dist::gather_checked)
  const std::vector<XYZZ<F>> all = dist::gather_checked<XYZZ<F>>(comm, [&] {
    if (!c) throw std::runtime_error("null MSM context");
    return c->run(bases, scalars, n);
  });
  XYZZ<F> acc = XYZZ<F>::zero();
  for (const auto& p : all) acc = acc + p;
  const Affine<F> a = acc.to_affine();
  memcpy(out, &a, sizeof(a));
}

#define CURVE_DISPATCH(curve, CALL)                               \
  switch (curve) {                                                \
    case 0: { using C = Bn254G1; CALL; } break;                   \
    case 1: { using C = Bn254G2; CALL; } break;                   \
    case 2: { using C = Bls381G1; CALL; } break;                  \
    case 3: { using C = Bls381G2; CALL; } break;                  \
    default: throw std::runtime_error("unknown curve id");        \
  }

// One rank's part of a tachyon_mi355x_msm_shard plan: its point group over
// its window range (the hybrid partition; a point shard when window_groups
// is 1), the all-gather of the XYZZ partials and their sum in rank order.
// The window-range partials sum_{w in range} 2^(c w) S_w of the Q ranges of
// one point group add up to that group's MSM, the groups' to the whole MSM.
// The exchanged record has one size on every curve (the largest XYZZ), so a
// rank whose plan or curve id is bad can still enter the all-gather with its
// failure flag: the plan is checked against the communicator and the curve's
// window count inside gather_checked's local part, before any local work.
struct ShardPartial {
  alignas(8) uint8_t bytes[sizeof(XYZZ<Bls381G2::F>)];
};

template <class Curve>
ShardPartial msm_shard_partial(void* ctx, dist::Comm* comm, const tachyon_mi355x_msm_shard& p, const void* bases,
                               const void* scalars) {
  using F = typename Curve::F;
  static_assert(sizeof(XYZZ<F>) <= sizeof(ShardPartial));
  auto* c = static_cast<MsmCtx<Curve>*>(ctx);
  if ((uint64_t)p.point_groups * p.window_groups != (uint64_t)comm->world())
    throw std::runtime_error("shard plan of " + std::to_string(p.point_groups) + " x " +
                             std::to_string(p.window_groups) + " ranks on a communicator of " +
                             std::to_string(comm->world()));
  if (p.w_begin > p.w_end) throw std::runtime_error("shard plan with w_begin > w_end");
  if (p.window_bits > 26) throw std::runtime_error("shard plan with more than 26 window bits");
  if (!c) throw std::runtime_error("null MSM context");
  const unsigned bits = p.window_bits ? p.window_bits : c->impl.force_window_bits();
  const unsigned W = msm::MsmPlan::make(p.count, Curve::Fr::Config::kModulusBits, bits).windows;
  if (p.w_end > W)
    throw std::runtime_error("shard plan with w_end " + std::to_string(p.w_end) + " above the " + std::to_string(W) +
                             " windows of its window bits");
  XYZZ<F> part;
  if (p.window_groups <= 1) {
    part = c->run(bases, scalars, p.count);
  } else {
    struct Restore {
      msm::MsmGpu<Curve>& m;
      unsigned c;
      ~Restore() { m.set_force_window_bits(c); }
    } restore{c->impl, c->impl.force_window_bits()};
    c->impl.set_force_window_bits(p.window_bits);
    part = c->impl.run_window_range(bases, scalars, p.count, p.w_begin, p.w_end);
  }
  ShardPartial out{};
  memcpy(out.bytes, &part, sizeof(part));
  return out;
}

template <class Curve>
void msm_shard_sum(const std::vector<ShardPartial>& all, void* out) {
  using F = typename Curve::F;
  XYZZ<F> acc = XYZZ<F>::zero();
  for (const ShardPartial& q : all) {
    XYZZ<F> v;
    memcpy(&v, q.bytes, sizeof(v));
    acc = acc + v;
  }
  const Affine<F> a = acc.to_affine();
  memcpy(out, &a, sizeof(a));
}

void msm_sharded_plan_out(int curve, void* ctx, dist::Comm* comm, const tachyon_mi355x_msm_shard* plan,
                          const void* bases, const void* scalars, void* out) {
  const std::vector<ShardPartial> all = dist::gather_checked<ShardPartial>(comm, [&]() -> ShardPartial {
    if (!plan) throw std::runtime_error("null shard plan");
    CURVE_DISPATCH(curve, return msm_shard_partial<C>(ctx, comm, *plan, bases, scalars))
    return ShardPartial{};
  });
  CURVE_DISPATCH(curve, msm_shard_sum<C>(all, out))
}

// The hybrid point x window partitions (curve id, world) -> (window groups Q,
// window bits c) that beat point shards on one MI355X (the slowest rank of
// each partition timed with the real kernels: BN254 G1 2^26 at 8 ranks 11.45
// vs 12.11 ms, profiles/r05c; BLS12-381 G2 2^24 at 4 / 8 ranks 31.16 / 17.21
// vs 32.19 / 17.81 ms, profiles/r05m); point shards everywhere else.
struct HybridPlan {
  int curve, world;
  unsigned q, c;
};
constexpr HybridPlan kHybridPlans[] = {{0, 8, 2, 19}, {3, 4, 2, 19}, {3, 8, 4, 16}};

template <class Curve>
void affine_sum(const void* pts, size_t count, void* out) {
  using F = typename Curve::F;
  const Affine<F>* p = static_cast<const Affine<F>*>(pts);
  XYZZ<F> acc = XYZZ<F>::zero();
  for (size_t i = 0; i < count; ++i) acc = acc.madd(p[i]);
  Affine<F> a = acc.to_affine();
  memcpy(out, &a, sizeof(a));
}

template <class Curve>
void jac_to_affine(const void* jac, void* out) {
  using F = typename Curve::F;
  Jacobian<F> j;
  memcpy(&j, jac, sizeof(j));
  Affine<F> a = XYZZ<F>::from_jacobian(j).to_affine();
  memcpy(out, &a, sizeof(a));
}

}  // namespace

struct tachyon_bn254_g1_msm : MsmCtx<Bn254G1> {};
struct tachyon_bn254_g1_msm_gpu : MsmCtx<Bn254G1> {};
struct tachyon_bls12_381_g1_msm : MsmCtx<Bls381G1> {};
struct tachyon_bls12_381_g1_msm_gpu : MsmCtx<Bls381G1> {};
struct tachyon_bn254_g2_msm_gpu : MsmCtx<Bn254G2> {};
struct tachyon_bls12_381_g2_msm_gpu : MsmCtx<Bls381G2> {};

extern "C" {

void tachyon_bn254_g1_init(void) {}
void tachyon_bls12_381_g1_init(void) {}
void tachyon_bn254_g2_init(void) {}
void tachyon_bls12_381_g2_init(void) {}

// ---- BN254 G1 ----
tachyon_bn254_g1_msm_ptr tachyon_bn254_g1_create_msm(uint8_t degree) {
  (void)degree;  // unused, as in msm.h:23
  GUARD_BEGIN return new tachyon_bn254_g1_msm(); GUARD_END
}
void tachyon_bn254_g1_destroy_msm(tachyon_bn254_g1_msm_ptr ptr) { delete ptr; }
tachyon_bn254_g1_jacobian* tachyon_bn254_g1_point2_msm(tachyon_bn254_g1_msm_ptr ptr,
                                                       const tachyon_bn254_g1_point2* bases,
                                                       const tachyon_bn254_fr* scalars, size_t size) {
  GUARD_BEGIN return do_msm<Bn254G1, tachyon_bn254_g1_jacobian>(ptr, bases, scalars, size); GUARD_END
}
tachyon_bn254_g1_jacobian* tachyon_bn254_g1_affine_msm(tachyon_bn254_g1_msm_ptr ptr,
                                                       const tachyon_bn254_g1_affine* bases,
                                                       const tachyon_bn254_fr* scalars, size_t size) {
  GUARD_BEGIN return do_msm<Bn254G1, tachyon_bn254_g1_jacobian>(ptr, bases, scalars, size); GUARD_END
}
tachyon_bn254_g1_msm_gpu_ptr tachyon_bn254_g1_create_msm_gpu(uint8_t degree) {
  (void)degree;
  GUARD_BEGIN return new tachyon_bn254_g1_msm_gpu(); GUARD_END
}
void tachyon_bn254_g1_destroy_msm_gpu(tachyon_bn254_g1_msm_gpu_ptr ptr) { delete ptr; }
tachyon_bn254_g1_jacobian* tachyon_bn254_g1_point2_msm_gpu(tachyon_bn254_g1_msm_gpu_ptr ptr,
                                                           const tachyon_bn254_g1_point2* bases,
                                                           const tachyon_bn254_fr* scalars, size_t size) {
  GUARD_BEGIN return do_msm<Bn254G1, tachyon_bn254_g1_jacobian>(ptr, bases, scalars, size); GUARD_END
}
tachyon_bn254_g1_jacobian* tachyon_bn254_g1_affine_msm_gpu(tachyon_bn254_g1_msm_gpu_ptr ptr,
                                                           const tachyon_bn254_g1_affine* bases,
                                                           const tachyon_bn254_fr* scalars, size_t size) {
  GUARD_BEGIN return do_msm<Bn254G1, tachyon_bn254_g1_jacobian>(ptr, bases, scalars, size); GUARD_END
}

// ---- BLS12-381 G1 ----
tachyon_bls12_381_g1_msm_ptr tachyon_bls12_381_g1_create_msm(uint8_t degree) {
  (void)degree;
  GUARD_BEGIN return new tachyon_bls12_381_g1_msm(); GUARD_END
}
void tachyon_bls12_381_g1_destroy_msm(tachyon_bls12_381_g1_msm_ptr ptr) { delete ptr; }
tachyon_bls12_381_g1_jacobian* tachyon_bls12_381_g1_point2_msm(tachyon_bls12_381_g1_msm_ptr ptr,
                                                               const tachyon_bls12_381_g1_point2* bases,
                                                               const tachyon_bls12_381_fr* scalars, size_t size) {
  GUARD_BEGIN return do_msm<Bls381G1, tachyon_bls12_381_g1_jacobian>(ptr, bases, scalars, size); GUARD_END
}
tachyon_bls12_381_g1_jacobian* tachyon_bls12_381_g1_affine_msm(tachyon_bls12_381_g1_msm_ptr ptr,
                                                               const tachyon_bls12_381_g1_affine* bases,
                                                               const tachyon_bls12_381_fr* scalars, size_t size) {
  GUARD_BEGIN return do_msm<Bls381G1, tachyon_bls12_381_g1_jacobian>(ptr, bases, scalars, size); GUARD_END
}
tachyon_bls12_381_g1_msm_gpu_ptr tachyon_bls12_381_g1_create_msm_gpu(uint8_t degree) {
  (void)degree;
  GUARD_BEGIN return new tachyon_bls12_381_g1_msm_gpu(); GUARD_END
}
void tachyon_bls12_381_g1_destroy_msm_gpu(tachyon_bls12_381_g1_msm_gpu_ptr ptr) { delete ptr; }
tachyon_bls12_381_g1_jacobian* tachyon_bls12_381_g1_point2_msm_gpu(tachyon_bls12_381_g1_msm_gpu_ptr ptr,
                                                                   const tachyon_bls12_381_g1_point2* bases,
                                                                   const tachyon_bls12_381_fr* scalars,
                                                                   size_t size) {
  GUARD_BEGIN return do_msm<Bls381G1, tachyon_bls12_381_g1_jacobian>(ptr, bases, scalars, size); GUARD_END
}
tachyon_bls12_381_g1_jacobian* tachyon_bls12_381_g1_affine_msm_gpu(tachyon_bls12_381_g1_msm_gpu_ptr ptr,
                                                                   const tachyon_bls12_381_g1_affine* bases,
                                                                   const tachyon_bls12_381_fr* scalars,
                                                                   size_t size) {
  GUARD_BEGIN return do_msm<Bls381G1, tachyon_bls12_381_g1_jacobian>(ptr, bases, scalars, size); GUARD_END
}

// ---- G2 (extension) ----
tachyon_bn254_g2_msm_gpu_ptr tachyon_bn254_g2_create_msm_gpu(uint8_t degree) {
  (void)degree;
  GUARD_BEGIN return new tachyon_bn254_g2_msm_gpu(); GUARD_END
}
void tachyon_bn254_g2_destroy_msm_gpu(tachyon_bn254_g2_msm_gpu_ptr ptr) { delete ptr; }
tachyon_bn254_g2_jacobian* tachyon_bn254_g2_affine_msm_gpu(tachyon_bn254_g2_msm_gpu_ptr ptr,
                                                           const tachyon_bn254_g2_affine* bases,
                                                           const tachyon_bn254_fr* scalars, size_t size) {
  GUARD_BEGIN return do_msm<Bn254G2, tachyon_bn254_g2_jacobian>(ptr, bases, scalars, size); GUARD_END
}
tachyon_bls12_381_g2_msm_gpu_ptr tachyon_bls12_381_g2_create_msm_gpu(uint8_t degree) {
  (void)degree;
  GUARD_BEGIN return new tachyon_bls12_381_g2_msm_gpu(); GUARD_END
}
void tachyon_bls12_381_g2_destroy_msm_gpu(tachyon_bls12_381_g2_msm_gpu_ptr ptr) { delete ptr; }
tachyon_bls12_381_g2_jacobian* tachyon_bls12_381_g2_affine_msm_gpu(tachyon_bls12_381_g2_msm_gpu_ptr ptr,
                                                                   const tachyon_bls12_381_g2_affine* bases,
                                                                   const tachyon_bls12_381_fr* scalars,
                                                                   size_t size) {
  GUARD_BEGIN return do_msm<Bls381G2, tachyon_bls12_381_g2_jacobian>(ptr, bases, scalars, size); GUARD_END
}

// ---- curve-generic extensions ----
// W of the uniform plan -- what a fold divides -- or 0 while mixed-width
// windows are set (a batch, a fold or a window range with them is refused)
static unsigned uniform_windows(int curve, const void* ctx, size_t size) {
  GUARD_BEGIN CURVE_DISPATCH(curve, {
    const auto& m = static_cast<const MsmCtx<C>*>(ctx)->impl;
    return m.mixed_windows() ? 0u : m.fold_windows(size);
  }) GUARD_END
  return 0;
}
// set_variant bits 2-3 = 1 or 2: one or two windows per sort group -- not a
// plain run, so refused together with mixed-width windows (3 = all windows in
// one group, the plain run's own grouping, is not)
static bool window_groups_set(int variant) {
  const int g = (variant >> 2) & 3;
  return g == 1 || g == 2;
}
void tachyon_mi355x_msm_gpu_affine(int curve, void* ctx, const void* bases, const void* scalars, size_t size,
                                   void* out_affine) {
  GUARD_BEGIN CURVE_DISPATCH(curve, msm_affine_out<C>(ctx, bases, scalars, size, out_affine)) GUARD_END
}
void tachyon_mi355x_msm_gpu_window_range_affine(int curve, void* ctx, const void* bases, const void* scalars,
                                                size_t size, unsigned w_begin, unsigned w_end, void* out_affine) {
  GUARD_BEGIN CURVE_DISPATCH(curve, msm_window_range_out<C>(ctx, bases, scalars, size, w_begin, w_end, out_affine))
  GUARD_END
}
int tachyon_mi355x_msm_gpu_batch_affine(int curve, void* ctx, const void* bases, size_t len, const void* scalars,
                                        size_t count, void* out_affine) {
  if (!is_device_pointer(bases) || (count > 1 && uniform_windows(curve, ctx, len) == 0)) return 0;
  GUARD_BEGIN CURVE_DISPATCH(curve, msm_batch_out<C>(ctx, bases, len, scalars, count, out_affine)) GUARD_END
  return 1;
}
unsigned tachyon_mi355x_msm_gpu_plan_windows(int curve, const void* ctx, size_t size) {
  GUARD_BEGIN CURVE_DISPATCH(curve, return static_cast<const MsmCtx<C>*>(ctx)->impl.plan_windows(size)) GUARD_END
  return 0;
}
int tachyon_mi355x_msm_gpu_fold_bases(int curve, void* ctx, const void* bases, size_t size, unsigned fold,
                                      void* out_bases) {
  if (fold == 0 || !is_device_pointer(bases) || !is_device_pointer(out_bases)) return 0;
  const unsigned W = uniform_windows(curve, ctx, size);
  if (W == 0 || W % fold != 0) return 0;  // refused, nothing written
  GUARD_BEGIN CURVE_DISPATCH(curve, static_cast<MsmCtx<C>*>(ctx)->impl.fold_bases(bases, size, fold, out_bases))
  GUARD_END
  return 1;
}
int tachyon_mi355x_msm_gpu_folded_affine(int curve, void* ctx, const void* folded_bases, const void* scalars,
                                         size_t size, unsigned fold, void* out_affine) {
  if (fold == 0 || !is_device_pointer(folded_bases) || !is_device_pointer(scalars)) return 0;
  const unsigned W = uniform_windows(curve, ctx, size);
  if (W == 0 || (fold > 1 && W % fold != 0)) return 0;
  GUARD_BEGIN CURVE_DISPATCH(curve, msm_folded_out<C>(ctx, folded_bases, scalars, size, fold, out_affine)) GUARD_END
  return 1;
}
void* tachyon_mi355x_msm_gpu_create(int curve, void* stream) {
  GUARD_BEGIN CURVE_DISPATCH(curve, return new MsmCtx<C>(static_cast<hipStream_t>(stream))) GUARD_END
  return nullptr;
}
void tachyon_mi355x_msm_gpu_destroy(int curve, void* ctx) {
  if (!ctx) return;
  GUARD_BEGIN CURVE_DISPATCH(curve, delete static_cast<MsmCtx<C>*>(ctx)) GUARD_END
}
int tachyon_mi355x_msm_gpu_run(int curve, void* ctx, const void* bases, size_t bases_size, const void* scalars,
                               size_t scalars_size, int form, void* out) {
  if (bases_size != scalars_size) return 0;  // IcicleMSM::Run / PippengerAdapter: sizes must match
  GUARD_BEGIN CURVE_DISPATCH(curve, msm_form_out<C>(ctx, bases, scalars, scalars_size, form, out)) GUARD_END
  return 1;
}
void tachyon_mi355x_msm_gpu_sharded_affine(int curve, void* ctx, tachyon_mi355x_comm* comm, const void* bases,
                                           const void* scalars, size_t size, void* out_affine) {
  GUARD_BEGIN
  if (!comm || !comm->impl) throw std::runtime_error("null communicator");
  CURVE_DISPATCH(curve, msm_sharded_out<C>(ctx, comm->impl.get(), bases, scalars, size, out_affine))
  GUARD_END
}
int tachyon_mi355x_msm_shard_plan(int curve, size_t n_total, int world, int rank, tachyon_mi355x_msm_shard* out) {
  if (!out || curve < 0 || curve > 3 || world < 1 || rank < 0 || rank >= world) return 0;
  unsigned q = 1, c = 0;
  for (const HybridPlan& h : kHybridPlans)
    if (h.curve == curve && h.world == world) {
      q = h.q;
      c = h.c;
    }
  const unsigned p = (unsigned)world / q;
  // point group rank / q: the ceil split of base::ParallelizeMap (dist.shard_range)
  const size_t chunk = (n_total + p - 1) / p;
  const size_t start = std::min<size_t>((size_t)(rank / q) * chunk, n_total);
  tachyon_mi355x_msm_shard s{};
  s.start = start;
  s.count = std::min(chunk, n_total - start);
  s.point_groups = p;
  s.window_groups = q;
  if (q > 1) {
    const unsigned bits = curve < 2 ? Bn254Fr::Config::kModulusBits : Bls381Fr::Config::kModulusBits;
    const unsigned W = (bits + 1 + c - 1) / c;
    const unsigned base = W / q, extra = W % q, j = (unsigned)rank % q;  // contiguous ranges (dist.window_range)
    s.window_bits = c;
    s.w_begin = j * base + std::min(j, extra);
    s.w_end = s.w_begin + base + (j < extra ? 1 : 0);
  }
  *out = s;
  return 1;
}
int tachyon_mi355x_msm_gpu_sharded_plan_affine(int curve, void* ctx, tachyon_mi355x_comm* comm,
                                               const tachyon_mi355x_msm_shard* plan, const void* bases,
                                               const void* scalars, void* out_affine) {
  // (no abort: a failure of any rank's local part reaches every rank through
  // the exchange, and every rank returns 0 with the message on stderr)
  return guarded_report(__func__, 0, [&] {
    if (!comm || !comm->impl) throw std::runtime_error("null communicator");
    // (a null plan, a bad curve id and a plan that does not match the
    // communicator fail inside the exchange, where every rank sees them)
    msm_sharded_plan_out(curve, ctx, comm->impl.get(), plan, bases, scalars, out_affine);
    return 1;
  });
}
int tachyon_mi355x_msm_gpu_run_points(int curve, void* ctx, const void* bases, size_t bases_size, int base_form,
                                      const void* scalars, size_t scalars_size, int form, void* out) {
  if (bases_size != scalars_size) return 0;
  GUARD_BEGIN CURVE_DISPATCH(curve, msm_points_form_out<C>(ctx, bases, base_form, scalars, scalars_size, form, out))
  GUARD_END
  return 1;
}
void tachyon_mi355x_msm_gpu_set_window_bits(int curve, void* ctx, unsigned c) {
  GUARD_BEGIN
  CURVE_DISPATCH(curve, static_cast<MsmCtx<C>*>(ctx)->set([&](auto& m) { m.set_force_window_bits(c); }))
  GUARD_END
}
int tachyon_mi355x_msm_gpu_set_mixed_windows(int curve, void* ctx, unsigned windows) {
  if (!ctx || curve < 0 || curve > 3) return 0;
  const unsigned bits = curve < 2 ? Bn254Fr::Config::kModulusBits : Bls381Fr::Config::kModulusBits;
  if (windows && !msm::MsmPlan::mixed_layout_ok(bits, windows)) return 0;  // refused, nothing changed
  GUARD_BEGIN
  CURVE_DISPATCH(curve, {
    auto* m = static_cast<MsmCtx<C>*>(ctx);
    if (windows && m->impl.force_window_bits()) return 0;  // not with forced window bits
    if (windows && window_groups_set(m->impl.variant())) return 0;  // nor with one or two windows per sort group
    m->set([&](auto& g) { g.set_mixed_windows(windows); });
  })
  GUARD_END
  return 1;
}
int tachyon_mi355x_msm_gpu_set_window_segment(int curve, void* ctx, unsigned length) {
  if (!ctx || curve < 0 || curve > 3) return 0;
  if (length && (length < 2 || length > 256 || (length & (length - 1)))) return 0;  // refused, nothing changed
  GUARD_BEGIN
  CURVE_DISPATCH(curve, static_cast<MsmCtx<C>*>(ctx)->set([&](auto& m) { m.set_window_segment(length); }))
  GUARD_END
  return 1;
}
int tachyon_mi355x_msm_mixed_layout(int curve, unsigned windows, unsigned* c_lo, unsigned* n_wide, unsigned* key_bits,
                                    unsigned* bit_offsets, unsigned* bucket_offsets) {
  if (curve < 0 || curve > 3) return 0;
  const unsigned bits = curve < 2 ? Bn254Fr::Config::kModulusBits : Bls381Fr::Config::kModulusBits;
  if (!msm::MsmPlan::mixed_layout_ok(bits, windows)) return 0;
  GUARD_BEGIN
  const msm::MsmPlan p = msm::MsmPlan::make_mixed(1, bits, windows);
  if (c_lo) *c_lo = p.c;
  if (n_wide) *n_wide = p.n_wide;
  if (key_bits) *key_bits = msm::kMixedKeyBits;
  for (unsigned w = 0; w <= windows; ++w) {
    if (bit_offsets) bit_offsets[w] = p.bit_offset(w);
    if (bucket_offsets) bucket_offsets[w] = (unsigned)p.bucket_offset(w);
  }
  GUARD_END
  return 1;
}
int tachyon_mi355x_msm_gpu_set_devices(int curve, void* ctx, const int* device_ids, size_t count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  for (size_t i = 0; i < count; ++i)
    if (device_ids[i] < 0 || device_ids[i] >= n) return 0;  // refused, nothing changed
  GUARD_BEGIN CURVE_DISPATCH(curve, {
    auto* m = static_cast<MsmCtx<C>*>(ctx);
    m->multi.reset();
    if (count > 1) {
      m->multi = std::make_unique<msm::MsmMultiDevice<C>>(std::vector<int>(device_ids, device_ids + count));
      m->multi->copy_settings(m->impl);  // window bits, variant and profiling forced before set_devices
    }
  }) GUARD_END
  return 1;
}
size_t tachyon_mi355x_msm_gpu_last_shards(int curve, const void* ctx, float* shard_ms, size_t* shard_points,
                                          int* shard_devices, size_t cap) {
  GUARD_BEGIN CURVE_DISPATCH(curve, {
    auto* m = static_cast<const MsmCtx<C>*>(ctx);
    if (!m->multi) return 0;
    const auto& ms = m->multi->last_shard_ms();
    const auto& np = m->multi->last_shard_points();
    const auto ids = m->multi->device_ids();
    for (size_t i = 0; i < ids.size() && i < cap; ++i) {
      if (shard_ms) shard_ms[i] = i < ms.size() ? ms[i] : 0.f;
      if (shard_points) shard_points[i] = i < np.size() ? np[i] : 0;
      if (shard_devices) shard_devices[i] = ids[i];
    }
    return ids.size();
  }) GUARD_END
  return 0;
}
void tachyon_mi355x_msm_gpu_set_profile(int curve, void* ctx, int on) {
  GUARD_BEGIN
  CURVE_DISPATCH(curve, static_cast<MsmCtx<C>*>(ctx)->set([&](auto& m) { m.set_profile(on != 0); }))
  GUARD_END
}
int tachyon_mi355x_msm_gpu_set_variant(int curve, void* ctx, int variant) {
  if (variant < 0 || (variant & ~msm::kMsmVariantMask)) return 0;  // unknown bits: refused, nothing changed
  GUARD_BEGIN
  CURVE_DISPATCH(curve, {
    auto* m = static_cast<MsmCtx<C>*>(ctx);
    // window groups while mixed-width windows are set: the next run would throw (refused, nothing changed)
    if (m->impl.mixed_windows() && window_groups_set(variant)) return 0;
    m->set([&](auto& g) { g.set_variant(variant); });
  })
  GUARD_END
  return 1;
}
void tachyon_mi355x_msm_gpu_last_timings(int curve, const void* ctx, float* out8) {
  GUARD_BEGIN CURVE_DISPATCH(curve, {
    const msm::MsmTimings& t = static_cast<const MsmCtx<C>*>(ctx)->lead().timings();
    out8[0] = t.h2d; out8[1] = t.recode; out8[2] = t.sort; out8[3] = t.prep; out8[4] = t.acc; out8[5] = t.reduce;
    out8[6] = t.total; out8[7] = t.acc_launches;
  }) GUARD_END
}
unsigned tachyon_mi355x_msm_gpu_last_schedule(int curve, const void* ctx) {
  GUARD_BEGIN CURVE_DISPATCH(curve, return static_cast<const MsmCtx<C>*>(ctx)->lead().last_schedule()) GUARD_END
  return 0;
}
double tachyon_mi355x_msm_madd_ceiling(int curve, int field_bits) {
  GUARD_BEGIN CURVE_DISPATCH(curve, return msm::MsmGpu<C>::madd_ceiling(field_bits)) GUARD_END
  return 0.0;
}
size_t tachyon_mi355x_msm_gpu_last_divisions(int curve, const void* ctx) {
  GUARD_BEGIN CURVE_DISPATCH(curve, {
    auto* m = static_cast<const MsmCtx<C>*>(ctx);
    return m->multi ? m->multi->last_divisions() : m->impl.last_divisions();
  }) GUARD_END
  return 0;
}
size_t tachyon_mi355x_msm_gpu_run_bytes(int curve, const void* ctx, size_t size, size_t batch_count) {
  if (!ctx) return 0;
  GUARD_BEGIN CURVE_DISPATCH(curve, {
    const msm::MsmGpu<C>& g = static_cast<const MsmCtx<C>*>(ctx)->lead();
    return batch_count ? g.batch_run_bytes(size, batch_count) : g.run_bytes(size);
  }) GUARD_END
  return 0;
}
size_t tachyon_mi355x_msm_gpu_held_bytes(int curve, const void* ctx) {
  if (!ctx) return 0;
  GUARD_BEGIN CURVE_DISPATCH(curve, return static_cast<const MsmCtx<C>*>(ctx)->lead().held_bytes()) GUARD_END
  return 0;
}
void tachyon_mi355x_msm_plan(int curve, size_t size, unsigned* c, unsigned* windows) {
  GUARD_BEGIN CURVE_DISPATCH(curve, {
    msm::MsmPlan p = msm::MsmGpu<C>::default_plan(size);  // (mixed widths: the narrow windows' bits)
    *c = p.c;
    *windows = p.windows;
  }) GUARD_END
}
void tachyon_mi355x_affine_sum(int curve, const void* points, size_t count, void* out_affine) {
  GUARD_BEGIN CURVE_DISPATCH(curve, affine_sum<C>(points, count, out_affine)) GUARD_END
}
void tachyon_mi355x_jacobian_to_affine(int curve, const void* jacobian, void* out_affine) {
  GUARD_BEGIN CURVE_DISPATCH(curve, jac_to_affine<C>(jacobian, out_affine)) GUARD_END
}
void tachyon_mi355x_jacobian_destroy(int curve, void* jac) {
  switch (curve) {
    case 0: delete static_cast<tachyon_bn254_g1_jacobian*>(jac); break;
    case 1: delete static_cast<tachyon_bn254_g2_jacobian*>(jac); break;
    case 2: delete static_cast<tachyon_bls12_381_g1_jacobian*>(jac); break;
    case 3: delete static_cast<tachyon_bls12_381_g2_jacobian*>(jac); break;
  }
}

}  // extern "C"
