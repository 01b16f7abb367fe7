// C-ABI of the log-derivative lookup's m(X) and phi(X) (include/
// tachyon_mi355x.h, "Log-derivative lookup").  Reference: tachyon/zk/lookup/
// log_derivative_halo2/prover_impl.h:99-155, 186-316; every refusal is decided
// in log_lookup_validate.h before any GPU call, and a failure after that
// returns 0 with a message: these entry points never abort.
#include "../../../include/tachyon_mi355x.h"

#include <cstring>
#include <mutex>
#include <vector>

#include "../plonk/log_lookup.h"
#include "capi_guard.h"
#include "log_lookup_validate.h"

using namespace tachyon_amd;

namespace {

std::mutex g_timings_mutex;
float g_last_ms[plonk::kLlPhases] = {};

// the phases [begin, end) of the last call of their kind
void keep_timings(const float* ms, int begin, int end) {
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  for (int i = begin; i < end; ++i) g_last_ms[i] = ms[i];
}

template <class Fr>
std::vector<typename plonk::LogLookup<Fr>::Lookup> typed(const tachyon_mi355x_log_lookup* lookups, size_t count) {
  std::vector<typename plonk::LogLookup<Fr>::Lookup> out(count);
  for (size_t l = 0; l < count; ++l)
    out[l] = {reinterpret_cast<const Fr* const*>(lookups[l].inputs), lookups[l].num_inputs,
              static_cast<const Fr*>(lookups[l].table)};
  return out;
}

template <class Fr>
void run_m_polys(size_t n, size_t u, const tachyon_mi355x_log_lookup* lookups, size_t count, void* const* out_m,
                 uint64_t* out_misses) {
  const auto list = typed<Fr>(lookups, count);
  require_gpu();
  OwnedStream stream;
  plonk::LogLookup<Fr> ll(stream.s);
  float ms[plonk::kLlPhases] = {};
  ll.m_polys(n, u, list.data(), count, reinterpret_cast<Fr* const*>(out_m), out_misses, ms);
  keep_timings(ms, 0, 2);
}

template <class Fr>
void run_grand_sums(size_t n, size_t u, const void* beta, const tachyon_mi355x_log_lookup* lookups,
                    const void* const* m, size_t count, const void* blinds, void* const* out_phi, void* out_totals) {
  const auto list = typed<Fr>(lookups, count);
  Fr b;
  memcpy(&b, beta, sizeof(Fr));
  require_gpu();
  OwnedStream stream;
  plonk::LogLookup<Fr> ll(stream.s);
  float ms[plonk::kLlPhases] = {};
  ll.grand_sums(n, u, b, list.data(), reinterpret_cast<const Fr* const*>(m), count, static_cast<const Fr*>(blinds),
                reinterpret_cast<Fr* const*>(out_phi), static_cast<Fr*>(out_totals), ms);
  keep_timings(ms, 2, plonk::kLlPhases);
}

}  // namespace

extern "C" {

int tachyon_mi355x_log_lookup_m_polys(int field, size_t n, size_t usable_rows,
                                      const tachyon_mi355x_log_lookup* lookups, size_t count, void* const* out_m,
                                      uint64_t* out_misses) {
  if (!ll_validate::check_m_polys(field, n, usable_rows, lookups, count, out_m)) return 0;
  if (count == 0) return 1;  // nothing to do, and no GPU needed for it
  return guarded_report(__func__, 0, [&] {
    if (field == 0) run_m_polys<Bn254Fr>(n, usable_rows, lookups, count, out_m, out_misses);
    else run_m_polys<Bls381Fr>(n, usable_rows, lookups, count, out_m, out_misses);
    return 1;
  });
}

int tachyon_mi355x_log_lookup_grand_sums(int field, size_t n, size_t usable_rows, const void* beta,
                                         const tachyon_mi355x_log_lookup* lookups, const void* const* m, size_t count,
                                         const void* blinds, void* const* out_phi, void* out_totals) {
  // the length of blinds is the caller's contract: n - usable_rows - 1 per phi
  if (!ll_validate::check_grand_sums(field, n, usable_rows, beta, lookups, m, count, blinds,
                                     ll_validate::shape_ok(field, n, usable_rows)
                                         ? ll_validate::blind_elems(n, usable_rows, count)
                                         : 0,
                                     out_phi))
    return 0;
  if (count == 0) return 1;
  return guarded_report(__func__, 0, [&] {
    if (field == 0) run_grand_sums<Bn254Fr>(n, usable_rows, beta, lookups, m, count, blinds, out_phi, out_totals);
    else run_grand_sums<Bls381Fr>(n, usable_rows, beta, lookups, m, count, blinds, out_phi, out_totals);
    return 1;
  });
}

size_t tachyon_mi355x_log_lookup_tile_rows(void) { return plonk::kLlTile; }

size_t tachyon_mi355x_log_lookup_work_bytes(size_t n, size_t max_inputs, size_t count) {
  return guarded_report(__func__, (size_t)0, [&]() -> size_t {
    if (n < 2 || n > ll_validate::kMaxRows || (n & (n - 1)) != 0 || max_inputs == 0) return 0;
    require_gpu();  // the sort's scratch is sized for the device
    return plonk::LogLookup<Bn254Fr>::work_bytes(n, max_inputs, count);  // the same for both fields
  });
}

void tachyon_mi355x_log_lookup_last_timings(float* out_ms) {
  if (!out_ms) return;
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  memcpy(out_ms, g_last_ms, sizeof(g_last_ms));
}

}  // extern "C"
