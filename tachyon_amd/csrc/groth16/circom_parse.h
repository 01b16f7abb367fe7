// The circom readers themselves: zkey_curve, parse_zkey and parse_wtns of
// circom_io.h.  Host-only C++ over untrusted bytes, so it lives apart from the
// kernels: groth16.hip includes it and instantiates the readers for the
// library, and check/circom_io_check.cc includes it to drive them on bad files
// under the sanitizers with no GPU.  zkey_curve is an ordinary (non-inline)
// function defined here: include this header in ONE translation unit of a
// program.
//
// What the readers refuse, always with a std::runtime_error whose text starts
// with "circom:" and always before anything is allocated by a count taken
// from the file:
//   * bad magic / version / prover type, a missing section, a section that
//     runs past the end of the file;
//   * moduli that are not the curve's, num_vars < num_public + 1 (in 64 bits:
//     num_public = 0xFFFFFFFF does not wrap), a domain size that is no power
//     of two;
//   * a point section, the coefficient section or the wtns data section that
//     holds fewer than count x element-size bytes (count arithmetic in 64
//     bits, compared with the bytes left in the section BEFORE any resize --
//     the reference never allocates here, it points into the mapped file,
//     zkey.h ReadPtr);
//   * a coefficient whose constraint is >= domain_size or whose signal is
//     >= num_vars (the CSR build and the kernels index by them).
// Values are NOT range-checked, as in the reference: a coefficient word or a
// wtns value >= r is taken mod r by the Montgomery conversion.
#pragma once
#include <utility>

#include "circom_io.h"

namespace tachyon_amd::circom {

namespace parse_detail {

inline void check_magic(ByteReader& rd, const char* magic, uint32_t want_version, const char* what) {
  const uint8_t* m = rd.ptr(4);
  if (memcmp(m, magic, 4) != 0) throw std::runtime_error(std::string("circom: not a ") + what + " file (bad magic)");
  uint32_t version = rd.read<uint32_t>();
  if (version != want_version)
    throw std::runtime_error(std::string("circom: unsupported ") + what + " version " + std::to_string(version));
}

inline const std::pair<size_t, size_t>& section(const std::map<uint32_t, std::pair<size_t, size_t>>& secs,
                                                uint32_t id) {
  auto it = secs.find(id);
  if (it == secs.end()) throw std::runtime_error("circom: missing section " + std::to_string(id));
  return it->second;
}

// `count` elements of `elem` bytes must still be in the reader: checked in 64
// bits (count < 2^32, elem < 2^32: no overflow) before the caller allocates
inline void need_elements(const ByteReader& rd, uint64_t count, uint64_t elem, const char* what) {
  if (count * elem > rd.remaining())
    throw std::runtime_error(std::string("circom: truncated file (") + what + ": " + std::to_string(count) +
                             " elements of " + std::to_string(elem) + " bytes, " +
                             std::to_string(rd.remaining()) + " bytes left in the section)");
}

template <class T>
void read_array(ByteReader& rd, std::vector<T>* out, size_t count, const char* what) {
  need_elements(rd, count, sizeof(T), what);
  out->resize(count);
  if (count) rd.take(out->data(), count * sizeof(T));
}

template <class F>
struct BaseCfgOf {
  using type = typename F::Config;
};
template <class B>
struct BaseCfgOf<Fp2<B>> {
  using type = typename B::Config;
};

}  // namespace parse_detail

CurveId zkey_curve(const uint8_t* data, size_t len) {
  using namespace parse_detail;
  ByteReader rd(data, len);
  check_magic(rd, "zkey", 1, "zkey");
  auto secs = read_sections(rd);
  auto [off, size] = section(secs, 2);
  ByteReader g(data + off, size);
  uint32_t n8q = g.read<uint32_t>();
  const uint8_t* q = g.ptr(n8q);
  if (modulus_matches<consts::bn254_fq>(q, n8q)) return CurveId::kBn254;
  if (modulus_matches<consts::bls12_381_fq>(q, n8q)) return CurveId::kBls12_381;
  throw std::runtime_error("circom: zkey base field is neither BN254 nor BLS12-381");
}

template <class G1, class G2>
ZKey<G1, G2> parse_zkey(const uint8_t* data, size_t len) {
  using namespace parse_detail;
  using Z = ZKey<G1, G2>;
  using Fr = typename Z::Fr;
  Z z;
  ByteReader rd(data, len);
  check_magic(rd, "zkey", 1, "zkey");
  auto secs = read_sections(rd);
  {
    auto [off, size] = section(secs, 1);  // header: prover type 1 = Groth16
    ByteReader h(data + off, size);
    if (h.read<uint32_t>() != 1) throw std::runtime_error("circom: zkey prover type is not Groth16");
  }
  {
    auto [off, size] = section(secs, 2);
    ByteReader g(data + off, size);
    uint32_t n8q = g.read<uint32_t>();
    if (!modulus_matches<typename BaseCfgOf<typename G1::F>::type>(g.ptr(n8q), n8q))
      throw std::runtime_error("circom: zkey base field does not match the curve");
    uint32_t n8r = g.read<uint32_t>();
    if (!modulus_matches<typename Fr::Config>(g.ptr(n8r), n8r))
      throw std::runtime_error("circom: zkey scalar field does not match the curve");
    z.num_vars = g.read<uint32_t>();
    z.num_public = g.read<uint32_t>();
    z.domain_size = g.read<uint32_t>();
    // (64 bits: num_public + 1 must not wrap to 0)
    if ((uint64_t)z.num_vars < (uint64_t)z.num_public + 1)
      throw std::runtime_error("circom: zkey has fewer variables than inputs");
    if (z.domain_size == 0 || (z.domain_size & (z.domain_size - 1)))
      throw std::runtime_error("circom: zkey domain size is not a power of two");
    z.alpha_g1 = g.read<typename Z::A1>();
    z.beta_g1 = g.read<typename Z::A1>();
    z.beta_g2 = g.read<typename Z::A2>();
    z.gamma_g2 = g.read<typename Z::A2>();
    z.delta_g1 = g.read<typename Z::A1>();
    z.delta_g2 = g.read<typename Z::A2>();
  }
  auto points = [&](uint32_t id, auto* out, size_t count, const char* what) {
    auto [off, size] = section(secs, id);
    ByteReader p(data + off, size);
    read_array(p, out, count, what);
  };
  points(3, &z.ic, z.num_instance(), "section 3, IC");
  {
    auto [off, size] = section(secs, 4);
    ByteReader c(data + off, size);
    uint32_t count = c.read<uint32_t>();
    need_elements(c, count, 3 * sizeof(uint32_t) + sizeof(Fr), "section 4, coefficients");
    z.coefficients.resize(count);
    for (uint32_t i = 0; i < count; ++i) {
      auto& e = z.coefficients[i];
      e.matrix = c.read<uint32_t>();
      e.constraint = c.read<uint32_t>();
      e.signal = c.read<uint32_t>();
      // the CSR build and qap_abc_kernel index by these two
      if (e.constraint >= z.domain_size)
        throw std::runtime_error("circom: coefficient constraint index outside the domain");
      if (e.signal >= z.num_vars) throw std::runtime_error("circom: coefficient signal index out of range");
      Fr raw;
      c.take(&raw, sizeof(Fr));
      // zkey.h:219-220: value = F::FromMontgomery(value.ToBigInt()), i.e. the
      // stored word times R^-1 becomes the Montgomery representation
      e.value = raw.from_mont();
    }
  }
  points(5, &z.a1, z.num_vars, "section 5, A");
  points(6, &z.b1, z.num_vars, "section 6, B1");
  points(7, &z.b2, z.num_vars, "section 7, B2");
  points(8, &z.c1, z.num_witness(), "section 8, C");
  points(9, &z.h1, z.domain_size, "section 9, H");
  return z;
}

template <class Fr>
std::vector<Fr> parse_wtns(const uint8_t* data, size_t len) {
  using namespace parse_detail;
  ByteReader rd(data, len);
  check_magic(rd, "wtns", 2, "wtns");
  auto secs = read_sections(rd);
  uint32_t count;
  {
    auto [off, size] = section(secs, 1);
    ByteReader h(data + off, size);
    uint32_t n8 = h.read<uint32_t>();
    if (!modulus_matches<typename Fr::Config>(h.ptr(n8), n8))
      throw std::runtime_error("circom: wtns field does not match the curve's scalar field");
    count = h.read<uint32_t>();
  }
  auto [off, size] = section(secs, 2);
  ByteReader d(data + off, size);
  need_elements(d, count, sizeof(Fr), "wtns section 2, values");
  std::vector<Fr> out(count);
  for (uint32_t i = 0; i < count; ++i) {
    Fr raw;
    d.take(&raw, sizeof(Fr));
    out[i] = raw.to_mont();  // wtns.h:116: F(witnesses[i].value()) -- canonical in, Montgomery out
  }
  return out;
}

}  // namespace tachyon_amd::circom
