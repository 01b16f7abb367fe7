"""CPU checks for the BabyBear NTT: the reference the GPU tests compare against
(tests/babybear_ref.py) agrees with the definitions it is written from, the
generated header carries the same constants, the holder header compiles for
BabyBear (and still for the 32-byte fields), and the built library exports the
two batch entry points."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import babybear_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = B.P
LIB = os.path.join(ROOT, "tachyon_amd", "libtachyon_mi355x.so")
CONSTANTS = os.path.join(ROOT, "tachyon_amd", "csrc", "field", "bb31_constants.h")


def rand(seed, *shape):
    return np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)


def test_constants():
    assert P == 2013265921 == 0x78000001
    assert B.R % P == 268435454
    assert B.R * B.R % P == 1172168163
    assert (-pow(P, -1, B.R)) % B.R == 2013265919
    assert (P - 1) == 15 << 27 and B.TWO_ADICITY == 27
    assert B.root_of_unity(1 << 27) == pow(31, 15, P) == 440564289 == 0x1A427A41
    assert B.from_mont(B.mont(12345)) == 12345


def test_generator_has_full_order():
    # p - 1 = 2^27 * 3 * 5: 31 has order p - 1 iff no 31^((p-1)/q) is 1
    assert pow(31, P - 1, P) == 1
    for q in (2, 3, 5):
        assert pow(31, (P - 1) // q, P) != 1
    for log_n in range(0, 28):
        w = B.root_of_unity(1 << log_n)
        assert pow(w, 1 << log_n, P) == 1 and (log_n == 0 or pow(w, 1 << (log_n - 1), P) == P - 1)


@pytest.mark.parametrize("log_n", range(0, 7))
def test_dft_is_direct_evaluation(log_n):
    n = 1 << log_n
    w = B.root_of_unity(n)
    x = rand(100 + log_n, n, 3)
    got = B.dft(x, w)
    for c in range(3):
        xs = [int(v) for v in x[:, c]]
        for i in range(n):
            assert int(got[i, c]) == sum(xs[j] * pow(w, i * j, P) for j in range(n)) % P
    assert (B.dft(x[:, 0], w) == got[:, 0]).all()  # a 1-D vector is one column


@pytest.mark.parametrize("log_n", [0, 1, 5, 10])
def test_round_trips(log_n):
    n = 1 << log_n
    for x in (rand(200 + log_n, n), rand(300 + log_n, n, 5), np.full((n, 2), P - 1, dtype=np.uint64)):
        assert (B.ifft(B.fft(x)) == x).all()
        assert (B.ifft(B.fft(x, 31), 31) == x).all()
        assert (B.fft(B.ifft(x, 7), 7) == x).all()
        if n > 1:
            assert not (B.fft(x, 31) == B.fft(x)).all()


@pytest.mark.parametrize("log_rows", range(0, 5))
@pytest.mark.parametrize("added", [0, 1, 3])
def test_coset_lde_is_the_interpolant_on_the_coset(log_rows, added):
    rows, cols, shift = 1 << log_rows, 3, 31
    x = rand(400 + log_rows, rows, cols)
    got = B.coset_lde(x, added, shift)
    big = rows << added
    w_small, w_big = B.root_of_unity(rows), B.root_of_unity(big)
    assert got.shape == (big, cols)
    for c in range(cols):
        # coefficients by the inverse DFT from its definition, then Horner
        ys = [int(v) for v in x[:, c]]
        inv = pow(rows, -1, P)
        coeffs = [sum(ys[i] * pow(w_small, -i * j, P) for i in range(rows)) * inv % P for j in range(rows)]
        for i in range(big):
            pt, acc = shift * pow(w_big, i, P) % P, 0
            for a in reversed(coeffs):
                acc = (acc * pt + a) % P
            assert int(got[i, c]) == acc


@pytest.mark.parametrize("added", [0, 1, 2, 3])
def test_coset_lde_with_shift_one_keeps_the_input_rows(added):
    x = rand(500 + added, 16, 4)
    out = B.coset_lde(x, added, 1)
    for i in range(16):
        assert (out[i << added] == x[i]).all()


def test_mont_words_commute_with_the_transform():
    # the transform of the Montgomery words is the Montgomery form of the transform
    x = rand(600, 32, 2)
    xm = x * np.uint64(B.R % P) % np.uint64(P)
    assert (B.fft(xm, 31) == B.fft(x, 31) * np.uint64(B.R % P) % np.uint64(P)).all()


def test_generated_header_matches():
    text = open(CONSTANTS).read()
    got = {k: int(v) for k, v in re.findall(r"uint32_t (k\w+) = (\d+)u;", text)}
    assert got == {
        "kP": P, "kR": B.R % P, "kR2": B.R * B.R % P, "kNInv": (-pow(P, -1, B.R)) % B.R, "kGenerator": 31,
        "kTwoAdicity": 27, "kRootOfUnity": B.root_of_unity(1 << 27),
        "kRootOfUnityMont": B.mont(B.root_of_unity(1 << 27)),
    }
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_bb31_constants.py"), "--check"])
    assert r.returncode == 0, "bb31_constants.h is stale: run tools/gen_bb31_constants.py"
    from tachyon_amd import params
    assert params.BABY_BEAR == P and params.baby_bear_root_of_unity(1 << 27) == B.root_of_unity(1 << 27)
    assert params.baby_bear_mont(31) == B.mont(31)


def test_host_field_arithmetic(tmp_path):
    """field/bb31.h on the host against Python integers, at the operand bounds
    (0, 1, p - 1) and on seeded words."""
    src = tmp_path / "bb31_host.cc"
    src.write_text('#include <cstdio>\n#include "bb31.h"\nusing namespace tachyon_amd::bb31;\n'
                   "int main() {\n  unsigned a, b;\n"
                   '  while (scanf("%u %u", &a, &b) == 2)\n'
                   '    printf("%u %u %u %u %u\\n", add(a, b), sub(a, b), mul(a, b), to_mont(a), from_mont(a));\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "bb31_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "tachyon_amd", "csrc", "field"), str(src), "-o", str(exe)], check=True)
    edge = [0, 1, 2, P - 1, P - 2, B.R % P, (P + 1) // 2]
    pairs = [(a, b) for a in edge for b in edge] + [tuple(int(v) for v in row) for row in rand(700, 200, 2)]
    out = subprocess.run([str(exe)], input="".join(f"{a} {b}\n" for a, b in pairs), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    rinv = pow(B.R, -1, P)
    for (a, b), line in zip(pairs, out):
        assert [int(v) for v in line.split()] == [(a + b) % P, (a - b) % P, a * b * rinv % P, a * B.R % P,
                                                  a * rinv % P], (a, b)


HOLDER_USE = r'''
#include "tachyon_mi355x_ntt_holder.h"
namespace math = tachyon_mi355x;
namespace ntt = tachyon_mi355x::ntt;
struct BabyBear { uint32_t value; };
struct BigInt1 { uint64_t limbs[1]; };
struct Evals { std::vector<BabyBear> v; const std::vector<BabyBear>& evaluations() const { return v; } };
struct Coeffs { std::vector<BabyBear> v; const std::vector<BabyBear>& coefficients() const { return v; } };
struct Poly { Coeffs c; const Coeffs& coefficients() const { return c; } };
bool f(const BabyBear& group_gen, const BigInt1& offset_big_int_, Evals& evals, Poly& poly, const BabyBear* in,
       BabyBear* out, const BabyBear& shift) {
  math::IcicleNTTHolder<BabyBear, math::kBabyBear> icicle_ntt_holder_ =
      math::IcicleNTTHolder<BabyBear, math::kBabyBear>::Create();
  if (!icicle_ntt_holder_->Init(group_gen)) return false;
  const math::IcicleNTTHolder<BabyBear, math::kBabyBear>* icicle_ = &icicle_ntt_holder_;
  return (*icicle_)->FFT(ntt::NttAlgorithm::Radix2, offset_big_int_, evals) &&
         (*icicle_)->IFFT(ntt::NttAlgorithm::Radix2, offset_big_int_, poly) &&
         (*icicle_)->FFTBatch(out, 8, 3) && (*icicle_)->CosetLDEBatch(in, 8, 3, 1, shift, out);
}
// the 32-byte fields as before
struct Fr { uint64_t limbs[4]; };
struct BigInt4 { uint64_t limbs[4]; };
struct Evals4 { std::vector<Fr> v; const std::vector<Fr>& evaluations() const { return v; } };
struct Coeffs4 { std::vector<Fr> v; const std::vector<Fr>& coefficients() const { return v; } };
struct Poly4 { Coeffs4 c; const Coeffs4& coefficients() const { return c; } };
template <int kField>
bool g(const Fr& group_gen, const BigInt4& offset, Evals4& evals, Poly4& poly) {
  auto holder = math::IcicleNTTHolder<Fr, kField>::Create();
  return holder->Init(group_gen) && holder->FFT(ntt::NttAlgorithm::Auto, offset, evals) &&
         holder->IFFT(ntt::NttAlgorithm::Auto, offset, poly);
}
template bool g<math::kBn254Fr>(const Fr&, const BigInt4&, Evals4&, Poly4&);
template bool g<math::kBls12_381Fr>(const Fr&, const BigInt4&, Evals4&, Poly4&);
'''


def compile_holder(tmp_path, text):
    src = tmp_path / "use_holder.cc"
    src.write_text(text)
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)


def test_holder_header_compiles_for_baby_bear_and_the_fr_fields(tmp_path):
    r = compile_holder(tmp_path, HOLDER_USE)
    assert r.returncode == 0, r.stderr


def test_holder_header_rejects_wrong_sizes(tmp_path):
    # a 32-byte element on kBabyBear, and a 4-byte one on kBn254Fr, do not compile
    for f, field in (("struct F { uint64_t l[4]; };", "kBabyBear"), ("struct F { uint32_t v; };", "kBn254Fr")):
        r = compile_holder(tmp_path, '#include "tachyon_mi355x_ntt_holder.h"\n' + f +
                           "\nbool h(const F& g) { auto x = tachyon_mi355x::IcicleNTTHolder<F, tachyon_mi355x::" +
                           field + ">::Create(); return x->Init(g); }\n")
        assert r.returncode != 0 and "element size" in r.stderr


def test_library_exports_the_batch_entries():
    if not os.path.exists(LIB):
        pytest.skip("libtachyon_mi355x.so not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert {"tachyon_mi355x_icicle_ntt_run_matrix", "tachyon_mi355x_icicle_ntt_coset_lde_batch"} <= exported
    from tachyon_amd._lib import SIGNATURES
    assert {"tachyon_mi355x_icicle_ntt_run_matrix", "tachyon_mi355x_icicle_ntt_coset_lde_batch"} <= \
        {n for n, _, _ in SIGNATURES}
