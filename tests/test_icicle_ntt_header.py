"""CPU-side checks of the drop-in IcicleNTT holder (no GPU):
include/tachyon_mi355x_ntt_holder.h compiles against stand-in F / BigInt /
Evals / DensePoly types with the reference's call lines written verbatim
(univariate_evaluation_domain.h:150-154,198-202, zk/base/entities/entity.h:90-93),
and the argument checks of the C-ABI (csrc/capi/icicle_ntt_validate.h) run as
a stand-alone host program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

USE_HOLDER = r"""
#include "tachyon_mi355x_ntt_holder.h"

#define CHECK(x) do { if (!(x)) __builtin_trap(); } while (0)
#define TACHYON_CUDA 1

namespace ntt = tachyon_mi355x::ntt;
namespace math {
template <class F>
using IcicleNTTHolder = tachyon_mi355x::IcicleNTTHolder<F, tachyon_mi355x::kBn254Fr>;
template <class F>
constexpr bool IsIcicleNTTSupported = true;
}  // namespace math
using math::IsIcicleNTTSupported;

struct BigInt { unsigned long long limbs[4]; };
struct Fr { using BigIntTy = BigInt; unsigned long long limbs[4]; };

struct Evals {
  std::vector<Fr> evaluations_;
  const std::vector<Fr>& evaluations() const { return evaluations_; }
};
struct Coefficients {
  std::vector<Fr> coefficients_;
  const std::vector<Fr>& coefficients() const { return coefficients_; }
};
struct DensePoly {
  Coefficients coefficients_;
  const Coefficients& coefficients() const { return coefficients_; }
};

enum class FFTAlgorithm { kRadix2, kMixedRadix };
constexpr ::ntt::NttAlgorithm FFTAlgorithmToIcicleNTTAlgorithm(FFTAlgorithm a) {
  return a == FFTAlgorithm::kRadix2 ? ::ntt::NttAlgorithm::Radix2 : ::ntt::NttAlgorithm::MixedRadix;
}

template <class F>
struct Domain {
  void set_icicle(const math::IcicleNTTHolder<F>* icicle) { icicle_ = icicle; }
  const F& group_gen() const { return group_gen_; }
  FFTAlgorithm GetAlgorithm() const { return FFTAlgorithm::kRadix2; }

  Evals FFT(const DensePoly& poly) const {
    Evals evals;
    evals.evaluations_ = poly.coefficients_.coefficients_;
#if TACHYON_CUDA
    // TODO(chokobole): Remove this condition.
    if constexpr (IsIcicleNTTSupported<F>) {
      if (icicle_) {
        evals.evaluations_.resize(size_);
        CHECK((*icicle_)->FFT(FFTAlgorithmToIcicleNTTAlgorithm(GetAlgorithm()),
                              offset_big_int_, evals));
        return evals;
      }
    }
#endif
    return evals;
  }

  DensePoly IFFT(const Evals& evals) const {
    DensePoly poly;
    poly.coefficients_.coefficients_ = evals.evaluations_;
#if TACHYON_CUDA
    // TODO(chokobole): Remove this condition.
    if constexpr (IsIcicleNTTSupported<F>) {
      if (icicle_) {
        poly.coefficients_.coefficients_.resize(size_);
        CHECK((*icicle_)->IFFT(FFTAlgorithmToIcicleNTTAlgorithm(GetAlgorithm()),
                               offset_big_int_, poly));
        return poly;
      }
    }
#endif
    return poly;
  }

  size_t size_ = 0;
  F group_gen_ = {};
  typename F::BigIntTy offset_big_int_ = {};
  const math::IcicleNTTHolder<F>* icicle_ = nullptr;
};

template <class F>
struct Entity {
  void EnableIcicleNTT() {
    if (icicle_ntt_holder_) {
    } else {
      icicle_ntt_holder_ = math::IcicleNTTHolder<F>::Create();
      CHECK(icicle_ntt_holder_->Init(extended_domain_->group_gen()));
      domain_->set_icicle(&icicle_ntt_holder_);
      extended_domain_->set_icicle(&icicle_ntt_holder_);
    }
  }
  std::unique_ptr<Domain<F>> domain_, extended_domain_;
  math::IcicleNTTHolder<F> icicle_ntt_holder_;
};

DensePoly f(Entity<Fr>& e, const DensePoly& p) {
  e.EnableIcicleNTT();
  tachyon_mi355x::IcicleNTTOptions options;
  options.batch_size = 2;
  options.ordering = ::ntt::Ordering::kNN;
  math::IcicleNTTHolder<Fr> other = math::IcicleNTTHolder<Fr>::Create();
  CHECK(other->Init(e.domain_->group_gen(), options));
  Fr* raw = nullptr;
  CHECK((*other).Run(::ntt::NttAlgorithm::Auto, BigInt{{1, 0, 0, 0}}, raw, 0, ::ntt::NTTDir::kInverse));
  CHECK(other->Release());
  math::IcicleNTTHolder<Fr> moved = std::move(other);
  moved.Release();
  return e.domain_->IFFT(e.extended_domain_->FFT(p));
}
"""

VALIDATE_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>

#include "capi/icicle_ntt_validate.h"

using namespace tachyon_amd::icicle_ntt;

static int fails = 0;
#define EXPECT(x) do { if (!(x)) { printf("FAILED: %s\n", #x); ++fails; } } while (0)

int main() {
  tachyon_mi355x_icicle_ntt_options o = default_options();
  EXPECT(options_ok(o) && o.fast_twiddles_mode == 1 && o.batch_size == 1);
  o.batch_size = 0; EXPECT(!options_ok(o));
  o.batch_size = -3; EXPECT(!options_ok(o));
  o = default_options(); o.columns_batch = 1; EXPECT(!options_ok(o));
  o = default_options(); o.ordering = 1; EXPECT(!options_ok(o));
  o = default_options(); o.are_inputs_on_device = 1; EXPECT(!options_ok(o));
  o.are_outputs_on_device = 1; EXPECT(options_ok(o));
  o.is_async = 1; o.fast_twiddles_mode = 0; o.batch_size = 7; EXPECT(options_ok(o));

  EXPECT(size_log(1, 0) == 0 && size_log(2, 0) == -1 && size_log(0, 10) == -1);
  EXPECT(size_log(3, 10) == -1 && size_log(48, 10) == -1 && size_log(1024, 10) == 10 && size_log(2048, 10) == -1);
  EXPECT(size_log(16, -1) == -1 && size_log(size_t(1) << 30, 30) == 30 && size_log(~size_t(0), 30) == -1);
  EXPECT(size_log(size_t(1) << 63, 30) == -1);

  // exactly 32 heap bytes: a read past the end is an ASan report
  const uint32_t p[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u,
                         0x30644e72u};
  std::vector<unsigned char> bytes(32, 0);
  uint32_t w[8];
  load_words(bytes.data(), w);
  EXPECT(is_zero(w) && !coset_ok(w, p));
  bytes[0] = 5;
  load_words(bytes.data(), w);
  EXPECT(w[0] == 5 && coset_ok(w, p));
  std::memcpy(bytes.data(), p, 32);
  load_words(bytes.data(), w);
  EXPECT(std::memcmp(w, p, 32) == 0 && !below(w, p) && !coset_ok(w, p));
  bytes[0] = 0;  // p - 1
  load_words(bytes.data(), w);
  EXPECT(below(w, p) && coset_ok(w, p));
  std::memset(bytes.data(), 0xff, 32);
  load_words(bytes.data(), w);
  EXPECT(!below(w, p) && !coset_ok(w, p));
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_icicle_ntt_holder_header_compiles_with_reference_lines(tmp_path):
    src = tmp_path / "use_icicle_holder.cc"
    src.write_text(USE_HOLDER)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_icicle_ntt_argument_checks_standalone_sanitized(tmp_path):
    src = tmp_path / "validate_main.cc"
    exe = tmp_path / "validate_main"
    src.write_text(VALIDATE_MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-static-libasan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tachyon_amd", "csrc"), "-o", str(exe),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
