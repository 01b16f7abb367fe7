// Host-only check of capi/log_lookup_validate.h (no library, no HIP): valid
// calls pass, each refusal of tachyon_mi355x_log_lookup_m_polys and
// tachyon_mi355x_log_lookup_grand_sums is refused, and nothing is
// dereferenced beyond the descriptor arrays (the columns here are small on
// purpose: a read of n elements from them would be out of bounds under a
// sanitizer).  Not part of `all`:
//   make ../bin/log_lookup_validate_check [CXX=... HOST_CHECK_FLAGS=-fsanitize=address,undefined]
#include <cstdio>
#include <vector>

#include "../capi/log_lookup_validate.h"

namespace {

namespace v = tachyon_amd::ll_validate;

struct Call {
  int field = 0;
  size_t n = 8, u = 5;
  unsigned char beta[32] = {1};
  // one element each: the checks compare addresses, they never read a column
  unsigned char in0[32] = {}, in1[32] = {}, in2[32] = {}, table0[32] = {}, table1[32] = {};
  unsigned char blinds[4 * 32] = {};
  std::vector<unsigned char> out0 = std::vector<unsigned char>(8 * 32), out1 = std::vector<unsigned char>(8 * 32);
  // away from the inputs: an output may be an m in the first call
  std::vector<unsigned char> m0 = std::vector<unsigned char>(8 * 32), m1 = std::vector<unsigned char>(8 * 32);
  const void* inputs0[2] = {in0, in1};
  const void* inputs1[1] = {in2};
  tachyon_mi355x_log_lookup lookups[2] = {};
  const void* m[2] = {};
  void* outs[2] = {};
  size_t num_blinds = 4;
  const void* beta_arg = beta;
  const tachyon_mi355x_log_lookup* lookups_arg = lookups;
  const void* const* m_arg = m;
  const void* blinds_arg = blinds;
  void* const* outs_arg = outs;

  Call() {
    lookups[0] = {inputs0, 2, table0};
    lookups[1] = {inputs1, 1, table1};
    outs[0] = out0.data();
    outs[1] = out1.data();
    m[0] = m0.data();
    m[1] = m1.data();
  }
  bool m_ok() const { return v::check_m_polys(field, n, u, lookups_arg, 2, outs_arg); }
  bool sums_ok() const {
    return v::check_grand_sums(field, n, u, beta_arg, lookups_arg, m_arg, 2, blinds_arg, num_blinds, outs_arg);
  }
};

int failures = 0;

void expect(bool want, bool got, const char* what) {
  if (want != got) {
    printf("FAIL: %s\n", what);
    ++failures;
  }
}

// refused by both entry points
template <class Damage>
void refused(const char* what, Damage damage) {
  Call c;
  damage(c);
  expect(false, c.m_ok(), what);
  expect(false, c.sums_ok(), what);
}

// refused by the grand sums, of no concern to the multiplicities
template <class Damage>
void sums_refused(const char* what, Damage damage) {
  Call c;
  damage(c);
  expect(true, c.m_ok(), what);
  expect(false, c.sums_ok(), what);
}

}  // namespace

int main() {
  expect(true, Call().m_ok(), "a valid m_polys call");
  expect(true, Call().sums_ok(), "a valid grand_sums call");
  refused("field 1", [](Call& c) { c.field = 1; });
  refused("field 3", [](Call& c) { c.field = 3; });
  refused("field -1", [](Call& c) { c.field = -1; });
  refused("n == 0", [](Call& c) { c.n = 0; });
  refused("n == 1", [](Call& c) { c.n = 1, c.u = 0; });
  refused("n == 12", [](Call& c) { c.n = 12; });
  refused("n == 2^31", [](Call& c) { c.n = (size_t)1 << 31; });
  refused("usable_rows == 0", [](Call& c) { c.u = 0, c.num_blinds = 14; });
  refused("usable_rows == n", [](Call& c) { c.u = c.n; });
  refused("usable_rows > n", [](Call& c) { c.u = c.n + 1; });
  refused("null lookups", [](Call& c) { c.lookups_arg = nullptr; });
  refused("a lookup without inputs", [](Call& c) { c.lookups[1].num_inputs = 0; });
  refused("null input list", [](Call& c) { c.lookups[0].inputs = nullptr; });
  refused("null input", [](Call& c) { c.inputs0[1] = nullptr; });
  refused("null table", [](Call& c) { c.lookups[1].table = nullptr; });
  refused("null outputs", [](Call& c) { c.outs_arg = nullptr; });
  refused("null output", [](Call& c) { c.outs[1] = nullptr; });
  refused("output == an input", [](Call& c) { c.outs[0] = c.in2; });
  refused("output inside a table", [](Call& c) { c.outs[1] = c.table0 + 16; });
  refused("output == another output", [](Call& c) { c.outs[1] = c.outs[0]; });
  refused("output ends inside another output", [](Call& c) { c.outs[1] = c.out0.data() + 32; });
  sums_refused("null beta", [](Call& c) { c.beta_arg = nullptr; });
  sums_refused("null m list", [](Call& c) { c.m_arg = nullptr; });
  sums_refused("null m", [](Call& c) { c.m[0] = nullptr; });
  sums_refused("null blinds", [](Call& c) { c.blinds_arg = nullptr; });
  sums_refused("one blind too few", [](Call& c) { c.num_blinds = 3; });
  sums_refused("one blind too many", [](Call& c) { c.num_blinds = 5; });
  sums_refused("output == m", [](Call& c) { c.outs[0] = c.m1.data(); });
  {  // blinds may be null when there is no blind row
    Call c;
    c.u = c.n - 1;
    c.blinds_arg = nullptr;
    c.num_blinds = 0;
    expect(true, c.sums_ok(), "no blind row");
  }
  {  // the smallest and the largest domain
    Call c;
    c.n = 2, c.u = 1, c.num_blinds = 0;
    expect(true, c.m_ok(), "n == 2");
    expect(true, c.sums_ok(), "n == 2");
    expect(true, v::shape_ok(2, (size_t)1 << 30, ((size_t)1 << 30) - 6), "n == 2^30");
  }
  expect(true, v::check_m_polys(0, 8, 5, nullptr, 0, nullptr), "no lookups");
  if (failures) return 1;
  printf("log_lookup_validate_check ok\n");
  return 0;
}
