// Host-only check of capi/grand_product_validate.h (no library, no HIP): a
// valid call passes, each refusal of tachyon_mi355x_grand_product_chains is
// refused, and nothing is dereferenced beyond the descriptor arrays (the
// columns here are small on purpose: a read of n elements from them would be
// out of bounds under a sanitizer).  Not part of `all`:
//   make ../bin/grand_product_validate_check [CXX=... HOST_CHECK_FLAGS=-fsanitize=address,undefined]
#include <cstdio>
#include <vector>

#include "../capi/grand_product_validate.h"

namespace {

using tachyon_amd::gp_validate::check;

struct Call {
  int field = 0;
  size_t n = 8, u = 5;
  unsigned char omega[32] = {1}, delta[32] = {1};
  const void* omega_arg = omega;
  const void* delta_arg = delta;
  // one element each: the checks compare addresses, they never read a column
  unsigned char values[32] = {}, table[32] = {}, blinds[64] = {};
  std::vector<unsigned char> z = std::vector<unsigned char>(8 * 32);
  tachyon_mi355x_gp_factor num[1] = {}, den[1] = {};
  tachyon_mi355x_gp_poly polys[1] = {};
  size_t lens[1] = {1};
  void* outs[1] = {};
  const tachyon_mi355x_gp_poly* polys_arg = polys;
  const size_t* lens_arg = lens;
  const void* blinds_arg = blinds;
  void* const* outs_arg = outs;

  Call() {
    num[0].values = values;
    num[0].kind = 2;
    num[0].label = 1;
    den[0].values = values;
    den[0].table = table;
    den[0].kind = 1;
    polys[0] = {num, 1, den, 1};
    outs[0] = z.data();
  }
  bool ok() const {
    return check(field, n, u, omega_arg, delta_arg, polys_arg, lens_arg, 1, blinds_arg, outs_arg, 1024,
                 (size_t)1 << 30);
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
  damage(c);
  expect(false, c.ok(), what);
}

}  // namespace

int main() {
  expect(true, Call().ok(), "a valid call");
  refused("field 1", [](Call& c) { c.field = 1; });
  refused("field 3", [](Call& c) { c.field = 3; });
  refused("n == 0", [](Call& c) { c.n = 0; });
  refused("usable_rows == n", [](Call& c) { c.u = c.n; });
  refused("n == 2^31", [](Call& c) { c.n = (size_t)1 << 31; });
  refused("null polys", [](Call& c) { c.polys_arg = nullptr; });
  refused("null chain_lens", [](Call& c) { c.lens_arg = nullptr; });
  refused("null blinds", [](Call& c) { c.blinds_arg = nullptr; });
  refused("null out_z", [](Call& c) { c.outs_arg = nullptr; });
  refused("null out_z[0]", [](Call& c) { c.outs[0] = nullptr; });
  refused("null omega with a label", [](Call& c) { c.omega_arg = nullptr; });
  refused("null delta with a label", [](Call& c) { c.delta_arg = nullptr; });
  refused("null numerator list", [](Call& c) { c.polys[0].num = nullptr; });
  refused("null denominator list", [](Call& c) { c.polys[0].den = nullptr; });
  refused("null values", [](Call& c) { c.num[0].values = nullptr; });
  refused("kind 3", [](Call& c) { c.den[0].kind = 3; });
  refused("kind 1 without a table", [](Call& c) { c.den[0].table = nullptr; });
  refused("a job without factors", [](Call& c) { c.polys[0].num_count = c.polys[0].den_count = 0; });
  refused("output == values", [](Call& c) { c.outs[0] = c.values; });
  refused("output inside the table", [](Call& c) { c.outs[0] = c.table + 16; });
  refused("too many tiles", [](Call& c) { c.lens[0] = ((size_t)1 << 30) + 1; });
  {  // blinds may be null when there is no blind row; omega / delta without a label factor
    Call c;
    c.u = c.n - 1;
    c.blinds_arg = nullptr;
    c.num[0].kind = 0;
    c.omega_arg = c.delta_arg = nullptr;
    expect(true, c.ok(), "no blinds, no label");
  }
  if (failures) return 1;
  printf("grand_product_validate_check ok\n");
  return 0;
}
