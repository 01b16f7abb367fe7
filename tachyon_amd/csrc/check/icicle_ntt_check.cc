// Exercise the drop-in holder of include/tachyon_mi355x_ntt_holder.h
// (IcicleNTTHolder<F, kField> / IcicleNTT<F, kField>) the way a Tachyon build
// uses math::IcicleNTTHolder<F>: Create() without a size, one Init with the
// generator of the largest domain (zk/base/entities/entity.h:90-93), then the
// dispatch lines of univariate_evaluation_domain.h:150-154,198-202 on
// containers of several sizes, plain and on the coset 5<w> (bn254) / 7<w>
// (bls12_381) given as the canonical BigInt.
//   icicle_ntt_check --gen <64 hex digits> [--field bn254|bls12_381]
//                    [--log-order N] [--dump file] step...
//   --gen: the generator of order 2^N, 32 Montgomery bytes (the caller
//          computes it; nothing comes from the library under test)
//   step:  f<log_m> or i<log_m> (FFT / IFFT of 2^log_m elements), then 'c'
//          (on the coset) and / or 'p' (input = the previous step's output
//          instead of a fresh seeded vector), e.g.  f7 f9c i9cp i7
// All steps run on ONE holder.  dump: per step, input then output (2^log_m
// 32-byte Montgomery elements each).  Prints one JSON line; exit 0 = every
// call returned true and every 'p' inverse of a forward step gave its input.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tachyon_mi355x_ntt_holder.h"

namespace {

struct Fr4 {
  uint64_t limbs[4];
};
struct BigInt4 {
  uint64_t limbs[4];
};

// stand-ins for UnivariateEvaluations / UnivariateDensePolynomial: the
// accessors IcicleNTT::FFT / IFFT read (icicle_ntt.h:72-86)
struct Evals {
  std::vector<Fr4> evaluations_;
  const std::vector<Fr4>& evaluations() const { return evaluations_; }
};
struct DenseCoefficients {
  std::vector<Fr4> coefficients_;
  const std::vector<Fr4>& coefficients() const { return coefficients_; }
};
struct DensePoly {
  DenseCoefficients coefficients_;
  const DenseCoefficients& coefficients() const { return coefficients_; }
};

struct Step {
  bool inverse = false, coset = false, prev = false;
  unsigned log_m = 0;
};

bool parse_step(const std::string& s, Step* st) {
  if (s.size() < 2 || (s[0] != 'f' && s[0] != 'i')) return false;
  st->inverse = s[0] == 'i';
  size_t i = 1;
  unsigned v = 0;
  while (i < s.size() && s[i] >= '0' && s[i] <= '9') v = v * 10 + (unsigned)(s[i++] - '0');
  if (i == 1 || v > 30) return false;
  st->log_m = v;
  for (; i < s.size(); ++i) {
    if (s[i] == 'c') st->coset = true;
    else if (s[i] == 'p') st->prev = true;
    else return false;
  }
  return true;
}

bool parse_hex32(const std::string& hex, Fr4* out) {
  if (hex.size() != 64) return false;
  unsigned char b[32];
  for (int i = 0; i < 32; ++i) {
    unsigned v = 0;
    if (sscanf(hex.c_str() + 2 * i, "%2x", &v) != 1) return false;
    b[i] = (unsigned char)v;
  }
  std::memcpy(out, b, 32);
  return true;
}

std::vector<Fr4> seeded(int field, uint64_t seed, size_t n) {
  Fr4* d = nullptr;
  if (hipMalloc(&d, n * sizeof(Fr4)) != hipSuccess) exit(2);
  tachyon_mi355x_gen_scalars(field, seed, 0, n, d, nullptr);
  std::vector<Fr4> v(n);
  if (hipMemcpy(v.data(), d, n * sizeof(Fr4), hipMemcpyDeviceToHost) != hipSuccess) exit(2);
  (void)hipFree(d);
  return v;
}

bool same(const std::vector<Fr4>& a, const std::vector<Fr4>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0;
}

template <int kField>
int run(const Fr4& gen, unsigned log_order, const std::vector<Step>& steps, const char* dump) {
  namespace math = tachyon_mi355x;
  namespace ntt = tachyon_mi355x::ntt;
  using F = Fr4;
  const BigInt4 one = {{1, 0, 0, 0}};
  const BigInt4 shift = {{kField == tachyon_mi355x::kBn254Fr ? 5u : 7u, 0, 0, 0}};

  math::IcicleNTTHolder<F, kField> icicle_ntt_holder_;
  if (icicle_ntt_holder_) return 2;  // default-constructed: empty
  icicle_ntt_holder_ = math::IcicleNTTHolder<F, kField>::Create();
  const bool init_ok = icicle_ntt_holder_->Init(gen);
  const math::IcicleNTTHolder<F, kField>* icicle_ = &icicle_ntt_holder_;
  const bool order_ok = (*icicle_)->log_order() == (int)log_order;

  FILE* f = dump ? fopen(dump, "wb") : nullptr;
  if (dump && !f) return 2;
  bool calls_ok = init_ok && order_ok, round_ok = true;
  std::vector<F> prev_in, prev_out;
  bool prev_forward = false, prev_coset = false;
  for (size_t s = 0; init_ok && s < steps.size(); ++s) {
    const Step& st = steps[s];
    const size_t size_ = size_t(1) << st.log_m;
    const BigInt4 offset_big_int_ = st.coset ? shift : one;
    std::vector<F> input = st.prev ? prev_out : seeded(kField, 0x1C1C0000ULL + s, size_);
    if (input.size() != size_) return 2;
    std::vector<F> output;
    if (!st.inverse) {
      Evals evals;
      evals.evaluations_ = input;
      evals.evaluations_.resize(size_);
      calls_ok = (*icicle_)->FFT(ntt::NttAlgorithm::Radix2, offset_big_int_, evals) && calls_ok;
      output = evals.evaluations_;
    } else {
      DensePoly poly;
      poly.coefficients_.coefficients_ = input;
      poly.coefficients_.coefficients_.resize(size_);
      calls_ok = (*icicle_)->IFFT(ntt::NttAlgorithm::Radix2, offset_big_int_, poly) && calls_ok;
      output = poly.coefficients_.coefficients_;
      if (st.prev && prev_forward && prev_coset == st.coset) round_ok = same(output, prev_in) && round_ok;
    }
    if (f) {
      fwrite(input.data(), sizeof(F), size_, f);
      fwrite(output.data(), sizeof(F), size_, f);
    }
    prev_in = input;
    prev_out = output;
    prev_forward = !st.inverse;
    prev_coset = st.coset;
  }
  if (f) fclose(f);
  const bool release_ok = init_ok && icicle_ntt_holder_->Release() && icicle_ntt_holder_->log_order() == -1;
  icicle_ntt_holder_.Release();
  const bool ok = calls_ok && round_ok && release_ok && !icicle_ntt_holder_;
  printf("{\"field\": \"%s\", \"log_order\": %u, \"steps\": %zu, \"init\": %s, \"calls\": %s, \"round_trips\": %s, "
         "\"release\": %s}\n",
         kField == tachyon_mi355x::kBn254Fr ? "bn254_fr" : "bls12_381_fr", log_order, steps.size(),
         init_ok && order_ok ? "true" : "false", calls_ok ? "true" : "false", round_ok ? "true" : "false",
         release_ok ? "true" : "false");
  return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  unsigned log_order = 12;
  const char* dump = nullptr;
  bool bls = false, have_gen = false;
  Fr4 gen = {};
  std::vector<Step> steps;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--dump" && i + 1 < argc) dump = argv[++i];
    else if (a == "--field" && i + 1 < argc) bls = std::string(argv[++i]) == "bls12_381";
    else if (a == "--log-order" && i + 1 < argc) log_order = (unsigned)atoi(argv[++i]);
    else if (a == "--gen" && i + 1 < argc) have_gen = parse_hex32(argv[++i], &gen);
    else {
      Step st;
      if (!parse_step(a, &st)) {
        fprintf(stderr, "icicle_ntt_check: bad step '%s'\n", a.c_str());
        return 2;
      }
      steps.push_back(st);
    }
  }
  if (!have_gen) {
    fprintf(stderr, "usage: icicle_ntt_check --gen <64 hex> [--field bn254|bls12_381] [--log-order N] [--dump file] "
                    "step...\n");
    return 2;
  }
  return bls ? run<tachyon_mi355x::kBls12_381Fr>(gen, log_order, steps, dump)
             : run<tachyon_mi355x::kBn254Fr>(gen, log_order, steps, dump);
}
