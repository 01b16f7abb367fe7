// Host-only check of common/omega_table.h and common/sections.h (no library,
// no HIP) over a toy prime field: the tables' size, the three-factor product
// against omega^j at the tables' seams, and the section packer's offsets
// against the sums the grand-product and quotient drivers need.  Not part of
// `all`:
//   make ../bin/omega_table_check [CXX=... HOST_CHECK_FLAGS=-fsanitize=address,undefined]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../common/omega_table.h"
#include "../common/sections.h"

namespace {

using namespace tachyon_amd;

int failures = 0;
void expect(bool ok, const char* what, size_t a = 0, size_t b = 0) {
  if (ok) return;
  printf("FAIL: %s (%zu, %zu)\n", what, a, b);
  ++failures;
}

// Integers mod 2^31 - 1
struct Toy {
  static constexpr uint64_t kP = 2147483647;
  uint64_t v;
  static Toy one() { return {1}; }
  Toy operator*(const Toy& o) const { return {v * o.v % kP}; }
  Toy canonical() const { return {v % kP}; }
  Toy pow(size_t e) const {
    Toy r = one(), b = *this;
    for (; e; e >>= 1, b = b * b)
      if (e & 1) r = r * b;
    return r;
  }
};

void check_tables(size_t n) {
  constexpr size_t kBlock = 256;
  const Toy omega{48271};
  const size_t size = omega_table_size(n, kBlock);
  expect(size == kBlock + 256 + (n + kBlock * 256 - 1) / (kBlock * 256), "omega_table_size", n, size);
  std::vector<Toy> tab(size, Toy{0});  // exactly the size: the sanitizer sees a write past it
  omega_table_fill(tab.data(), n, kBlock, omega);
  for (size_t j : {size_t(0), size_t(255), size_t(256), size_t(65535), size_t(65536), n - 1}) {
    if (j >= n) continue;
    const size_t slab = j / kBlock;
    const Toy got = tab[j % kBlock] * (tab[kBlock + slab % kOmegaTabB] * tab[kBlock + kOmegaTabB + slab / kOmegaTabB]);
    expect(got.v == omega.pow(j).v, "A[j % block] B[(j / block) % 256] C[j / (block 256)] = omega^j", n, j);
  }
}

size_t by_hand_align16(size_t x) { return (x + 15) & ~size_t(15); }

void check_packer() {
  SectionPacker up;
  // the grand product's [jobs | factors | chains | omega tables | blinds]:
  // 3 jobs of 24 bytes, 5 factors of 88, 2 chains of 8, 513 table elements and 3 x 2 blinds of 32
  const size_t jobs = 3 * 24, factors = 5 * 88, chains = 2 * 8, tables = 513 * 32, blinds = 6 * 32;
  const size_t off_fac = by_hand_align16(jobs), off_chain = by_hand_align16(off_fac + factors);
  const size_t off_tab = by_hand_align16(off_chain + chains), off_blind = off_tab + tables;
  expect(up.add(jobs) == 0, "the first section starts the image");
  expect(up.add(factors) == off_fac, "grand product: factors", off_fac);
  expect(up.add(chains) == off_chain, "grand product: chains", off_chain);
  expect(up.add(tables) == off_tab, "grand product: tables", off_tab);
  expect(up.add(blinds) == off_blind, "grand product: blinds", off_blind);
  expect(up.size() == off_blind + blinds, "grand product: the image's size", up.size());
  expect(off_fac % 16 == 0 && off_chain % 16 == 0 && off_tab % 16 == 0 && off_blind % 16 == 0, "16-byte offsets");
  unsigned char* image = up.image();
  image[up.size() - 1] = 1;  // the image holds its last byte
  expect(up.data() == image && image[0] == 0, "the image is zeroed and stays where it is");

  // the quotient's per group [code | constants | column pointers], then the
  // tables: a group of 13 instructions of 12 bytes, 5 constants, 9 columns,
  // and one of a single instruction with no constant and no column
  up.reset();
  const size_t shape[2][3] = {{13 * 12, 5 * 32, 9 * 8}, {12, 0, 0}};
  size_t at = 0;
  for (const auto& g : shape) {
    expect(up.add(g[0]) == at, "quotient: code", at);
    at = by_hand_align16(at + g[0]);
    expect(up.add(g[1]) == at, "quotient: constants", at);
    at = by_hand_align16(at + g[1]);
    expect(up.add(g[2]) == at, "quotient: column pointers", at);
    at = by_hand_align16(at + g[2]);
  }
  expect(up.add(tables) == at && up.size() == at + tables, "quotient: tables and the image's size", at, up.size());

  // sections of no bytes share the next one's offset; an image of none is still an address
  up.reset();
  expect(up.add(0) == 0 && up.add(0) == 0 && up.size() == 0, "empty sections");
  expect(up.image() != nullptr, "an empty image");
  expect(up.add(5) == 0 && up.add(0) == 16 && up.add(1) == 16 && up.size() == 17, "an empty section between two");
}

}  // namespace

int main() {
  for (size_t n : {size_t(1), size_t(255), size_t(256), size_t(257), size_t(65535), size_t(65536), size_t(65537),
                   (size_t(1) << 17) + 3})
    check_tables(n);
  check_packer();
  if (failures == 0) printf("omega_table_check ok\n");
  return failures ? 1 : 0;
}
