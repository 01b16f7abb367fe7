// Host-only check of the circom readers (groth16/circom_parse.h: zkey_curve,
// parse_zkey, parse_wtns) on valid and on damaged files: no library, no HIP
// call, no GPU.  tests/test_circom_io_check.py writes the files, runs this
// program under the address and undefined-behaviour sanitizers and compares
// what it prints with oracle/circom_format.py.  The field headers use amdgcn
// builtins in host-visible templates, so the host compiler is hipcc's.  Not
// part of `all`:
//   make ../bin/circom_io_check [HOST_CHECK_FLAGS=-fsanitize=address,undefined]
//
//   circom_io_check zkey <curve> <file>...       one verdict line per file and, when it parsed, a dump
//   circom_io_check wtns <curve> <file>...       likewise (values as canonical integers)
//       both end with "peak_rss_kib N", the process's own peak resident set
//   circom_io_check prefixes <zkey|wtns> <curve> <file>    every proper prefix of the file
//   circom_io_check mutate <curve> <zkey file> <begin> <end> [<begin> <end>]...
//       every byte of the ranges set to 0x00, 0xFF, value - 1 and value + 1
// <curve> is bn254 or bls12_381: the instantiation asked to read the file.
// A verdict is "parsed", "refused: circom: ..." (the readers' own refusal) or
// "error: ..." (any other exception: a bare STL message is not a refusal).
// Every input is copied into a heap block of exactly its length, so the
// sanitizer sees a read one byte past it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "../groth16/circom_parse.h"

namespace {

using namespace tachyon_amd;
using namespace tachyon_amd::circom;

enum class Verdict { kParsed, kRefused, kError };

struct Bytes {
  std::unique_ptr<uint8_t[]> p;
  size_t n = 0;
};

Bytes exact_copy(const uint8_t* src, size_t n) {
  Bytes b;
  b.p.reset(new uint8_t[n]);
  if (n) memcpy(b.p.get(), src, n);
  b.n = n;
  return b;
}

bool read_file(const char* path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + got);
  fclose(f);
  return true;
}

void hex(const char* name, const void* data, size_t bytes) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  printf("%s ", name);
  for (size_t i = 0; i < bytes; ++i) printf("%02x", p[i]);
  printf("\n");
}

template <class T>
void hex_vec(const char* name, const std::vector<T>& v) {
  hex(name, v.data(), v.size() * sizeof(T));
}

// runs `fn`, returns the verdict and its text
template <class Fn>
Verdict guarded(Fn&& fn, std::string* text) {
  try {
    fn();
    *text = "parsed";
    return Verdict::kParsed;
  } catch (const std::runtime_error& e) {
    if (strncmp(e.what(), "circom:", 7) == 0) {
      *text = std::string("refused: ") + e.what();
      return Verdict::kRefused;
    }
    *text = std::string("error: ") + e.what();
  } catch (const std::exception& e) {
    *text = std::string("error: ") + e.what();
  }
  return Verdict::kError;
}

template <class G1, class G2>
void dump_zkey(const ZKey<G1, G2>& z) {
  using Fr = typename G1::Fr;
  printf("counts %u %u %u\n", z.num_vars, z.num_public, z.domain_size);
  hex("alpha_g1", &z.alpha_g1, sizeof(z.alpha_g1));
  hex("beta_g1", &z.beta_g1, sizeof(z.beta_g1));
  hex("beta_g2", &z.beta_g2, sizeof(z.beta_g2));
  hex("gamma_g2", &z.gamma_g2, sizeof(z.gamma_g2));
  hex("delta_g1", &z.delta_g1, sizeof(z.delta_g1));
  hex("delta_g2", &z.delta_g2, sizeof(z.delta_g2));
  hex_vec("ic", z.ic);
  hex_vec("a1", z.a1);
  hex_vec("b1", z.b1);
  hex_vec("b2", z.b2);
  hex_vec("c1", z.c1);
  hex_vec("h1", z.h1);
  for (const auto& e : z.coefficients) {
    const Fr v = e.value.from_mont();  // the canonical integer the prover multiplies by
    printf("coef %u %u %u ", e.matrix, e.constraint, e.signal);
    hex("", &v, sizeof(v));
  }
}

template <class G1, class G2>
Verdict zkey_file(const uint8_t* data, size_t len, bool dump, std::string* text) {
  ZKey<G1, G2> z;
  const Verdict v = guarded([&] { z = parse_zkey<G1, G2>(data, len); }, text);
  if (dump) {
    printf("%s\n", text->c_str());
    if (v == Verdict::kParsed) {
      std::string ctext;
      CurveId id = CurveId::kBn254;
      if (guarded([&] { id = zkey_curve(data, len); }, &ctext) == Verdict::kParsed)
        printf("curve %s\n", id == CurveId::kBn254 ? "bn254" : "bls12_381");
      else
        printf("curve %s\n", ctext.c_str());
      dump_zkey(z);
    }
    printf("end\n");
  }
  return v;
}

template <class Fr>
Verdict wtns_file(const uint8_t* data, size_t len, bool dump, std::string* text) {
  std::vector<Fr> w;
  const Verdict v = guarded([&] { w = parse_wtns<Fr>(data, len); }, text);
  if (dump) {
    printf("%s\n", text->c_str());
    if (v == Verdict::kParsed) {
      printf("count %zu\n", w.size());
      for (auto& x : w) x = x.from_mont();
      hex_vec("values", w);
    }
    printf("end\n");
  }
  return v;
}

Verdict read_one(bool zkey, bool bls, const uint8_t* data, size_t len, bool dump, std::string* text) {
  if (zkey) {
    return bls ? zkey_file<Bls381G1, Bls381G2>(data, len, dump, text)
               : zkey_file<Bn254G1, Bn254G2>(data, len, dump, text);
  }
  return bls ? wtns_file<Bls381Fr>(data, len, dump, text) : wtns_file<Bn254Fr>(data, len, dump, text);
}

// this process's own peak resident set (VmHWM, KiB; 0 where /proc has none):
// unlike the parent's wait4 figure it does not start from the parent's size
size_t peak_rss_kib() {
  FILE* f = fopen("/proc/self/status", "r");
  if (!f) return 0;
  char line[256];
  size_t kib = 0;
  while (fgets(line, sizeof(line), f))
    if (strncmp(line, "VmHWM:", 6) == 0) kib = strtoull(line + 6, nullptr, 10);
  fclose(f);
  return kib;
}

int usage() {
  fprintf(stderr, "usage: circom_io_check zkey|wtns <curve> <file>... | prefixes zkey|wtns <curve> <file> | "
                  "mutate <curve> <zkey> <begin> <end>...\n");
  return 2;
}

bool curve_arg(const char* s, bool* bls) {
  if (strcmp(s, "bn254") == 0) return *bls = false, true;
  if (strcmp(s, "bls12_381") == 0) return *bls = true, true;
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return usage();
  const std::string mode = argv[1];
  std::string text;
  if (mode == "zkey" || mode == "wtns") {
    bool bls;
    if (!curve_arg(argv[2], &bls)) return usage();
    int errors = 0;
    for (int i = 3; i < argc; ++i) {
      std::vector<uint8_t> file;
      if (!read_file(argv[i], &file)) return fprintf(stderr, "cannot read %s\n", argv[i]), 2;
      Bytes b = exact_copy(file.data(), file.size());
      printf("file %s\n", argv[i]);
      if (read_one(mode == "zkey", bls, b.p.get(), b.n, true, &text) == Verdict::kError) ++errors;
    }
    printf("peak_rss_kib %zu\n", peak_rss_kib());
    return errors ? 1 : 0;
  }
  if (mode == "prefixes") {
    if (argc != 5) return usage();
    const std::string kind = argv[2];
    bool bls;
    if ((kind != "zkey" && kind != "wtns") || !curve_arg(argv[3], &bls)) return usage();
    std::vector<uint8_t> file;
    if (!read_file(argv[4], &file)) return fprintf(stderr, "cannot read %s\n", argv[4]), 2;
    size_t refused = 0;
    for (size_t len = 0; len < file.size(); ++len) {
      Bytes b = exact_copy(file.data(), len);
      const Verdict v = read_one(kind == "zkey", bls, b.p.get(), b.n, false, &text);
      if (v == Verdict::kRefused) ++refused;
      else printf("prefix %zu %s\n", len, text.c_str());
    }
    printf("prefixes %zu refused %zu\n", file.size(), refused);
    return refused == file.size() ? 0 : 1;
  }
  if (mode == "mutate") {
    if (argc < 6 || (argc - 4) % 2) return usage();
    bool bls;
    if (!curve_arg(argv[2], &bls)) return usage();
    std::vector<uint8_t> file;
    if (!read_file(argv[3], &file)) return fprintf(stderr, "cannot read %s\n", argv[3]), 2;
    Bytes b = exact_copy(file.data(), file.size());
    size_t total = 0, parsed = 0, refused = 0, errors = 0;
    for (int a = 4; a + 1 < argc; a += 2) {
      const size_t begin = strtoull(argv[a], nullptr, 10), end = strtoull(argv[a + 1], nullptr, 10);
      if (begin > end || end > b.n) return usage();
      for (size_t at = begin; at < end; ++at) {
        const uint8_t was = b.p[at];
        const uint8_t tries[4] = {0x00, 0xFF, (uint8_t)(was - 1), (uint8_t)(was + 1)};
        for (uint8_t t : tries) {
          if (t == was) continue;
          b.p[at] = t;
          ++total;
          const Verdict v = read_one(true, bls, b.p.get(), b.n, false, &text);
          if (v == Verdict::kParsed) ++parsed;
          else if (v == Verdict::kRefused) ++refused;
          else ++errors, printf("mutation %zu %02x %s\n", at, t, text.c_str());
        }
        b.p[at] = was;
      }
    }
    printf("mutations %zu parsed %zu refused %zu errors %zu\n", total, parsed, refused, errors);
    return errors ? 1 : 0;
  }
  return usage();
}
