// Exercise IcicleNTTHolder<BabyBear, kBabyBear> of
// include/tachyon_mi355x_ntt_holder.h the way a Tachyon build uses
// math::IcicleNTTHolder<BabyBear>: Create() without a size, one Init with the
// generator of the largest domain, then the dispatch lines of
// univariate_evaluation_domain.h:150-154,198-202 on containers of several
// sizes, plain and on the coset 31<w> given as the canonical BigInt<1>, and
// the two batch calls on row-major matrices.  Only the header is used.
//   baby_bear_ntt_check --gen <Montgomery word, decimal> [--dump file] step...
//   --gen: the generator of order 2^LN as a Montgomery word (the caller
//          computes it; nothing comes from the library under test)
//   step:  f<L>[c]          FFT of 2^L elements ('c': on the coset 31)
//          i<L>[c]          IFFT
//          m<L>x<cols>      FFTBatch on a 2^L x cols matrix
//          l<L>x<cols>+<a>  CosetLDEBatch, added_bits a, shift 31
// All steps run on ONE holder.  dump: per step, input words then output words
// (uint32, Montgomery).  Prints one JSON line; exit 0 = every call returned
// true.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tachyon_mi355x_ntt_holder.h"

namespace {

constexpr uint32_t kP = 0x78000001u;

struct BabyBear {
  uint32_t value;
};
struct BigInt1 {
  uint64_t limbs[1];
};

// stand-ins for UnivariateEvaluations / UnivariateDensePolynomial: the
// accessors IcicleNTT::FFT / IFFT read (icicle_ntt.h:72-86)
struct Evals {
  std::vector<BabyBear> evaluations_;
  const std::vector<BabyBear>& evaluations() const { return evaluations_; }
};
struct DenseCoefficients {
  std::vector<BabyBear> coefficients_;
  const std::vector<BabyBear>& coefficients() const { return coefficients_; }
};
struct DensePoly {
  DenseCoefficients coefficients_;
  const DenseCoefficients& coefficients() const { return coefficients_; }
};

struct Step {
  char kind = 'f';
  bool coset = false;
  unsigned log_m = 0, cols = 1, added = 0;
};

bool number(const std::string& s, size_t* i, unsigned* v) {
  const size_t start = *i;
  *v = 0;
  while (*i < s.size() && s[*i] >= '0' && s[*i] <= '9') *v = *v * 10 + (unsigned)(s[(*i)++] - '0');
  return *i > start;
}

bool parse_step(const std::string& s, Step* st) {
  if (s.size() < 2 || !strchr("fiml", s[0])) return false;
  st->kind = s[0];
  size_t i = 1;
  if (!number(s, &i, &st->log_m) || st->log_m > 27) return false;
  if (st->kind == 'f' || st->kind == 'i') {
    if (i < s.size() && s[i] == 'c') st->coset = true, ++i;
    return i == s.size();
  }
  if (i >= s.size() || s[i++] != 'x' || !number(s, &i, &st->cols) || st->cols == 0) return false;
  if (st->kind == 'l') {
    if (i >= s.size() || s[i++] != '+' || !number(s, &i, &st->added)) return false;
  }
  return i == s.size();
}

// seeded words in [0, p) (splitmix64; the dump carries them to the checker)
std::vector<BabyBear> seeded(uint64_t seed, size_t n) {
  std::vector<BabyBear> v(n);
  uint64_t x = seed;
  for (size_t i = 0; i < n; ++i) {
    x += 0x9e3779b97f4a7c15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    v[i].value = (uint32_t)(z % kP);
  }
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  namespace math = tachyon_mi355x;
  namespace ntt = tachyon_mi355x::ntt;
  using F = BabyBear;
  const char* dump = nullptr;
  bool have_gen = false;
  F gen = {0};
  std::vector<Step> steps;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--dump" && i + 1 < argc) dump = argv[++i];
    else if (a == "--gen" && i + 1 < argc) gen.value = (uint32_t)strtoul(argv[++i], nullptr, 10), have_gen = true;
    else {
      Step st;
      if (!parse_step(a, &st)) {
        fprintf(stderr, "baby_bear_ntt_check: bad step '%s'\n", a.c_str());
        return 2;
      }
      steps.push_back(st);
    }
  }
  if (!have_gen) {
    fprintf(stderr, "usage: baby_bear_ntt_check --gen <Montgomery word> [--dump file] step...\n");
    return 2;
  }

  const BigInt1 one = {{1}};
  const BigInt1 shift = {{31}};
  const F shift_mont = {(uint32_t)((31ULL << 32) % kP)};

  math::IcicleNTTHolder<F, math::kBabyBear> icicle_ntt_holder_;
  if (icicle_ntt_holder_) return 2;  // default-constructed: empty
  icicle_ntt_holder_ = math::IcicleNTTHolder<F, math::kBabyBear>::Create();
  const bool init_ok = icicle_ntt_holder_->Init(gen);
  const math::IcicleNTTHolder<F, math::kBabyBear>* icicle_ = &icicle_ntt_holder_;

  FILE* f = dump ? fopen(dump, "wb") : nullptr;
  if (dump && !f) return 2;
  bool calls_ok = init_ok;
  for (size_t s = 0; init_ok && s < steps.size(); ++s) {
    const Step& st = steps[s];
    const size_t size_ = size_t(1) << st.log_m;
    const BigInt1 offset_big_int_ = st.coset ? shift : one;
    const std::vector<F> input = seeded(0xBB310000ULL + s, size_ * st.cols);
    std::vector<F> output;
    if (st.kind == 'f') {
      Evals evals;
      evals.evaluations_ = input;
      calls_ok = (*icicle_)->FFT(ntt::NttAlgorithm::Radix2, offset_big_int_, evals) && calls_ok;
      output = evals.evaluations_;
    } else if (st.kind == 'i') {
      DensePoly poly;
      poly.coefficients_.coefficients_ = input;
      calls_ok = (*icicle_)->IFFT(ntt::NttAlgorithm::Radix2, offset_big_int_, poly) && calls_ok;
      output = poly.coefficients_.coefficients_;
    } else if (st.kind == 'm') {
      output = input;
      calls_ok = (*icicle_)->FFTBatch(output.data(), size_, st.cols) && calls_ok;
    } else {
      output.assign((size_ << st.added) * st.cols, F{0});
      calls_ok = (*icicle_)->CosetLDEBatch(input.data(), size_, st.cols, st.added, shift_mont, output.data()) &&
                 calls_ok;
    }
    if (f) {
      fwrite(input.data(), sizeof(F), input.size(), f);
      fwrite(output.data(), sizeof(F), output.size(), f);
    }
  }
  if (f) fclose(f);
  const int log_order = init_ok ? icicle_ntt_holder_->log_order() : -1;
  const bool release_ok = init_ok && icicle_ntt_holder_->Release() && icicle_ntt_holder_->log_order() == -1;
  icicle_ntt_holder_.Release();
  const bool ok = calls_ok && release_ok && !icicle_ntt_holder_;
  printf("{\"field\": \"baby_bear\", \"log_order\": %d, \"steps\": %zu, \"init\": %s, \"calls\": %s, \"release\": %s}\n",
         log_order, steps.size(), init_ok ? "true" : "false", calls_ok ? "true" : "false",
         release_ok ? "true" : "false");
  return ok ? 0 : 1;
}
