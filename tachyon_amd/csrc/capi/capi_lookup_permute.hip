// C-ABI of the Halo2 lookup's permuted columns A' and S' (include/
// tachyon_mi355x.h, "Halo2 lookup: the permuted columns").  Reference:
// tachyon/zk/lookup/halo2/permute_expression_pair.h:29-142; every refusal is
// decided in lookup_permute_validate.h before any GPU call, and a failure
// after that returns 0 with a message: these entry points never abort.
#include "../../../include/tachyon_mi355x.h"

#include <cstring>
#include <mutex>
#include <vector>

#include "../plonk/lookup_permute.h"
#include "capi_guard.h"
#include "lookup_permute_validate.h"

using namespace tachyon_amd;

namespace {

std::mutex g_timings_mutex;
float g_last_ms[plonk::kLpPhases] = {};

template <class Fr>
void run_permute_pairs(size_t n, size_t u, const tachyon_mi355x_lookup_pair* pairs, size_t count, const void* blinds,
                       void* const* out_input, void* const* out_table, uint64_t* out_misses) {
  std::vector<typename plonk::LookupPermute<Fr>::Pair> list(count);
  for (size_t l = 0; l < count; ++l)
    list[l] = {static_cast<const Fr*>(pairs[l].input), static_cast<const Fr*>(pairs[l].table)};
  require_gpu();
  OwnedStream stream;
  plonk::LookupPermute<Fr> lp(stream.s);
  float ms[plonk::kLpPhases] = {};
  lp.permute_pairs(n, u, list.data(), count, static_cast<const Fr*>(blinds), reinterpret_cast<Fr* const*>(out_input),
                   reinterpret_cast<Fr* const*>(out_table), out_misses, ms);
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  memcpy(g_last_ms, ms, sizeof(g_last_ms));
}

}  // namespace

extern "C" {

int tachyon_mi355x_lookup_permute_pairs(int field, size_t n, size_t usable_rows,
                                        const tachyon_mi355x_lookup_pair* pairs, size_t count, const void* blinds,
                                        void* const* out_input, void* const* out_table, uint64_t* out_misses) {
  // the length of blinds is the caller's contract, 2 (n - usable_rows) per pair: the signature carries no count, so
  // the count the validator compares is its own (behind shape_ok only because n - usable_rows must not underflow)
  if (!lp_validate::check_permute_pairs(field, n, usable_rows, pairs, count, blinds,
                                        lp_validate::shape_ok(field, n, usable_rows)
                                            ? lp_validate::blind_elems(n, usable_rows, count)
                                            : 0,
                                        out_input, out_table))
    return 0;
  if (count == 0) return 1;  // nothing to do, and no GPU needed for it
  return guarded_report(__func__, 0, [&] {
    if (field == 0) run_permute_pairs<Bn254Fr>(n, usable_rows, pairs, count, blinds, out_input, out_table, out_misses);
    else run_permute_pairs<Bls381Fr>(n, usable_rows, pairs, count, blinds, out_input, out_table, out_misses);
    return 1;
  });
}

size_t tachyon_mi355x_lookup_permute_work_bytes(size_t n, size_t count) {
  return guarded_report(__func__, (size_t)0, [&]() -> size_t {
    if (n < 2 || n > lp_validate::kMaxRows || (n & (n - 1)) != 0) return 0;
    require_gpu();  // the sort's scratch is sized for the device
    return plonk::LookupPermute<Bn254Fr>::work_bytes(n, count);  // the same for both fields
  });
}

void tachyon_mi355x_lookup_permute_last_timings(float* out_ms) {
  if (!out_ms) return;
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  memcpy(out_ms, g_last_ms, sizeof(g_last_ms));
}

}  // extern "C"
