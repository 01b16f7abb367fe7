// Host-only check of capi/lookup_permute_validate.h (no library, no HIP): a
// valid call passes, each refusal of tachyon_mi355x_lookup_permute_pairs is
// refused, and nothing is dereferenced beyond the descriptor and pointer
// arrays (the columns here are small on purpose: a read of n elements from
// them would be out of bounds under a sanitizer).  Not part of `all`:
//   make ../bin/lookup_permute_validate_check [CXX=... HOST_CHECK_FLAGS=-fsanitize=address,undefined]
#include <cstdio>
#include <vector>

#include "../capi/lookup_permute_validate.h"

namespace {

namespace v = tachyon_amd::lp_validate;

struct Call {
  int field = 0;
  size_t n = 8, u = 5, count = 2;
  // one element each: the checks compare addresses, they never read a column
  unsigned char in0[32] = {}, in1[32] = {}, table0[32] = {}, table1[32] = {};
  unsigned char blinds[12 * 32] = {};
  std::vector<unsigned char> a0 = std::vector<unsigned char>(8 * 32), a1 = std::vector<unsigned char>(8 * 32);
  std::vector<unsigned char> s0 = std::vector<unsigned char>(8 * 32), s1 = std::vector<unsigned char>(8 * 32);
  tachyon_mi355x_lookup_pair pairs[2] = {};
  void* out_a[2] = {};
  void* out_s[2] = {};
  size_t num_blinds = 12;  // 2 pairs x 2 columns x (n - u)
  const tachyon_mi355x_lookup_pair* pairs_arg = pairs;
  const void* blinds_arg = blinds;
  void* const* out_a_arg = out_a;
  void* const* out_s_arg = out_s;

  Call() {
    pairs[0] = {in0, table0};
    pairs[1] = {in1, table1};
    out_a[0] = a0.data(), out_a[1] = a1.data();
    out_s[0] = s0.data(), out_s[1] = s1.data();
  }
  bool ok() const {
    return v::check_permute_pairs(field, n, u, pairs_arg, count, blinds_arg, num_blinds, out_a_arg, out_s_arg);
  }
};

int failures = 0;

void expect(bool want, bool got, const char* what) {
  if (want != got) {
    printf("FAIL: %s\n", what);
    ++failures;
  }
}

template <class Damage>
void refused(const char* what, Damage damage) {
  Call c;
  expect(true, c.ok(), "the call before the damage");
  damage(c);
  expect(false, c.ok(), what);
}

}  // namespace

int main() {
  expect(true, Call().ok(), "a valid call");
  refused("field 1", [](Call& c) { c.field = 1; });
  refused("field 3", [](Call& c) { c.field = 3; });
  refused("field -1", [](Call& c) { c.field = -1; });
  refused("n == 0", [](Call& c) { c.n = 0; });
  refused("n == 1", [](Call& c) { c.n = 1, c.u = 0; });
  refused("n == 12", [](Call& c) { c.n = 12, c.num_blinds = 28; });
  refused("n == 2^31", [](Call& c) { c.n = (size_t)1 << 31; });
  refused("usable_rows == 0", [](Call& c) { c.u = 0, c.num_blinds = 32; });
  refused("usable_rows == n", [](Call& c) { c.u = c.n, c.num_blinds = 0; });
  refused("usable_rows > n", [](Call& c) { c.u = c.n + 1; });
  refused("null pairs", [](Call& c) { c.pairs_arg = nullptr; });
  refused("null input", [](Call& c) { c.pairs[1].input = nullptr; });
  refused("null table", [](Call& c) { c.pairs[0].table = nullptr; });
  refused("null input outputs", [](Call& c) { c.out_a_arg = nullptr; });
  refused("null table outputs", [](Call& c) { c.out_s_arg = nullptr; });
  refused("null input output", [](Call& c) { c.out_a[1] = nullptr; });
  refused("null table output", [](Call& c) { c.out_s[0] = nullptr; });
  refused("A' == an input", [](Call& c) { c.out_a[0] = c.in1; });
  refused("S' == its own table", [](Call& c) { c.out_s[1] = c.table1; });
  refused("S' inside another pair's table", [](Call& c) { c.out_s[1] = c.table0 + 16; });
  refused("A' == another A'", [](Call& c) { c.out_a[1] = c.out_a[0]; });
  refused("S' == another S'", [](Call& c) { c.out_s[1] = c.out_s[0]; });
  refused("A' == its own S'", [](Call& c) { c.out_a[0] = c.out_s[0]; });
  refused("S' ends inside another pair's A'", [](Call& c) { c.out_s[0] = c.a1.data() + 32; });
  refused("null blinds", [](Call& c) { c.blinds_arg = nullptr; });
  refused("one blind too few", [](Call& c) { c.num_blinds = 11; });
  refused("one blind too many", [](Call& c) { c.num_blinds = 13; });
  refused("the blinds of one column only", [](Call& c) { c.num_blinds = 6; });
  {  // the smallest and the largest domain
    Call c;
    c.n = 2, c.u = 1, c.num_blinds = 4;
    expect(true, c.ok(), "n == 2");
    expect(true, v::shape_ok(2, (size_t)1 << 30, ((size_t)1 << 30) - 6), "n == 2^30");
  }
  {  // one pair whose input is its table: columns may coincide, outputs may not
    Call c;
    c.count = 1, c.num_blinds = 6;
    c.pairs[0].table = c.in0;
    expect(true, c.ok(), "input == table");
  }
  // no pairs: nothing to do is no refusal, and blinds may then be null
  expect(true, v::check_permute_pairs(0, 8, 5, nullptr, 0, nullptr, 0, nullptr, nullptr), "no pairs");
  expect(false, v::check_permute_pairs(0, 8, 5, nullptr, 0, nullptr, 1, nullptr, nullptr), "no pairs, one blind");
  if (failures) return 1;
  printf("lookup_permute_validate_check ok\n");
  return 0;
}
