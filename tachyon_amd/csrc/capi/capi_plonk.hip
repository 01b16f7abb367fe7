// C-ABI of the Halo2 grand products and quotient (include/tachyon_mi355x.h,
// "PLONK grand products", "PLONK quotient"; the quotient's refusals are
// decided in plonk/quotient_plan.h).  Reference: tachyon/zk/plonk/permutation/
// grand_product_argument.h:17-122 and its three callers; every refusal is
// decided in grand_product_validate.h before any GPU call, and a failure
// after that returns 0 with a message: this entry point never aborts.
#include "../../../include/tachyon_mi355x.h"

#include <cstring>
#include <mutex>
#include <vector>

#include "../plonk/grand_product.h"
#include "../plonk/quotient.h"
#include "capi_guard.h"
#include "grand_product_validate.h"

using namespace tachyon_amd;

namespace {

std::mutex g_timings_mutex;
float g_last_ms[3] = {0.f, 0.f, 0.f};

template <class Fr>
void run_chains(size_t n, size_t u, const void* omega, const void* delta, const tachyon_mi355x_gp_poly* polys,
                const size_t* chain_lens, size_t num_chains, const void* blinds, void* const* out_z, void* out_last) {
  using GP = plonk::GrandProduct<Fr>;
  size_t num_polys = 0;
  for (size_t c = 0; c < num_chains; ++c) num_polys += chain_lens[c];
  // the factor lists in the class's types (the constants copied out of the byte arrays)
  std::vector<std::vector<typename GP::Factor>> lists(2 * num_polys);
  std::vector<typename GP::Poly> jobs(num_polys);
  for (size_t i = 0; i < num_polys; ++i) {
    for (int side = 0; side < 2; ++side) {
      const tachyon_mi355x_gp_factor* f = side ? polys[i].den : polys[i].num;
      const size_t cnt = side ? polys[i].den_count : polys[i].num_count;
      auto& list = lists[2 * i + side];
      list.resize(cnt);
      for (size_t k = 0; k < cnt; ++k) {
        list[k].values = static_cast<const Fr*>(f[k].values);
        list[k].table = static_cast<const Fr*>(f[k].table);
        list[k].kind = f[k].kind;
        list[k].label = f[k].label;
        memcpy(&list[k].m, f[k].m, sizeof(Fr));
        memcpy(&list[k].c, f[k].c, sizeof(Fr));
      }
    }
    jobs[i] = {lists[2 * i].data(), lists[2 * i].size(), lists[2 * i + 1].data(), lists[2 * i + 1].size()};
  }
  Fr w = Fr::one(), d = Fr::one();
  if (omega) memcpy(&w, omega, sizeof(Fr));
  if (delta) memcpy(&d, delta, sizeof(Fr));
  require_gpu();
  OwnedStream stream;
  GP gp(stream.s);
  float ms[3];
  gp.run(n, u, w, d, jobs.data(), chain_lens, num_chains, static_cast<const Fr*>(blinds),
         reinterpret_cast<Fr* const*>(out_z), static_cast<Fr*>(out_last), ms);
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  memcpy(g_last_ms, ms, sizeof(ms));
}

namespace qp = quotient_plan;

float g_quotient_ms[plonk::kQPhases] = {};
size_t g_quotient_held = 0;

uint32_t two_adicity(int field) {
  return field == 0 ? (uint32_t)Bn254Fr::Config::kTwoAdicity : (uint32_t)Bls381Fr::Config::kTwoAdicity;
}

void keep_timings(const float* ms, size_t held, bool set_held) {
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  memcpy(g_quotient_ms, ms, sizeof(g_quotient_ms));
  if (set_held) g_quotient_held = held;
}

template <class Fr>
void quotient_part(const qp::Params& params, const qp::Table& table, const qp::Group& group, void* acc) {
  require_gpu();
  OwnedStream stream;
  plonk::Quotient<Fr> q(stream.s);
  float ms[plonk::kQPhases];
  q.evaluate_part(params, table, group, acc, ms);
  keep_timings(ms, 0, false);
}

template <class Fr>
void quotient_h(const qp::Params& params, const qp::System& system, const qp::Circuit* circuits, size_t num_circuits,
                const void* zeta, const void* delta, const void* ext_gen, int full, void* out) {
  Fr z, d = Fr::one(), g = Fr::one();
  memcpy(&z, zeta, sizeof(Fr));
  if (delta) memcpy(&d, delta, sizeof(Fr));
  if (ext_gen) memcpy(&g, ext_gen, sizeof(Fr));
  require_gpu();
  OwnedStream stream;
  plonk::Quotient<Fr> q(stream.s);
  float ms[plonk::kQPhases];
  q.h_poly(params, system, circuits, num_circuits, z, d, ext_gen ? &g : nullptr, full != 0, out, ms);
  keep_timings(ms, q.held_bytes(), true);
}

}  // namespace

extern "C" {

int tachyon_mi355x_grand_product_chains(int field, size_t n, size_t usable_rows, const void* omega, const void* delta,
                                        const tachyon_mi355x_gp_poly* polys, const size_t* chain_lens,
                                        size_t num_chains, const void* blinds, void* const* out_z, void* out_last) {
  if (!gp_validate::check(field, n, usable_rows, omega, delta, polys, chain_lens, num_chains, blinds, out_z,
                          plonk::kGpTile, plonk::kGpMaxTiles))
    return 0;
  return guarded_report(__func__, 0, [&] {
    if (field == 0)
      run_chains<Bn254Fr>(n, usable_rows, omega, delta, polys, chain_lens, num_chains, blinds, out_z, out_last);
    else
      run_chains<Bls381Fr>(n, usable_rows, omega, delta, polys, chain_lens, num_chains, blinds, out_z, out_last);
    return 1;
  });
}

size_t tachyon_mi355x_grand_product_tile_rows(void) { return plonk::kGpTile; }

size_t tachyon_mi355x_grand_product_walk_tiles(void) { return plonk::kGpWalk; }

void tachyon_mi355x_grand_product_last_timings(float* out_ms) {
  if (!out_ms) return;
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  memcpy(out_ms, g_last_ms, sizeof(g_last_ms));
}

int tachyon_mi355x_quotient_evaluate_part(const tachyon_mi355x_quotient_params* params,
                                          const tachyon_mi355x_quotient_table* table,
                                          const tachyon_mi355x_quotient_group* group, void* acc) {
  return guarded_report(__func__, 0, [&] {  // the validation allocates: inside the guard
    if (!params || !qp::part_ok(params, table, group, acc, two_adicity(params->field))) return 0;
    if (params->field == 0) quotient_part<Bn254Fr>(*params, *table, *group, acc);
    else quotient_part<Bls381Fr>(*params, *table, *group, acc);
    return 1;
  });
}

int tachyon_mi355x_quotient_h_poly(const tachyon_mi355x_quotient_params* params,
                                   const tachyon_mi355x_quotient_system* system,
                                   const tachyon_mi355x_quotient_circuit* circuits, size_t num_circuits,
                                   const void* zeta, const void* delta, const void* ext_gen, int full, void* out) {
  return guarded_report(__func__, 0, [&] {
    if (!params ||
        !qp::h_poly_ok(params, system, circuits, num_circuits, zeta, delta, out, two_adicity(params->field)))
      return 0;
    if (params->field == 0)
      quotient_h<Bn254Fr>(*params, *system, circuits, num_circuits, zeta, delta, ext_gen, full, out);
    else
      quotient_h<Bls381Fr>(*params, *system, circuits, num_circuits, zeta, delta, ext_gen, full, out);
    return 1;
  });
}

size_t tachyon_mi355x_quotient_work_bytes(const tachyon_mi355x_quotient_params* params,
                                          const tachyon_mi355x_quotient_system* system,
                                          const tachyon_mi355x_quotient_circuit* circuits, size_t num_circuits) {
  // the shape alone: zeta, delta and the output do not enter the estimate
  static const unsigned char kOne[32] = {1};
  return guarded_report(__func__, (size_t)0, [&]() -> size_t {
    if (!params ||
        !qp::h_poly_ok(params, system, circuits, num_circuits, kOne, kOne, kOne, two_adicity(params->field)))
      return 0;
    return params->field == 0 ? plonk::Quotient<Bn254Fr>::work_bytes(*params, *system, circuits, num_circuits)
                              : plonk::Quotient<Bls381Fr>::work_bytes(*params, *system, circuits, num_circuits);
  });
}

int tachyon_mi355x_quotient_program_stats(const tachyon_mi355x_quotient_params* params,
                                          const tachyon_mi355x_quotient_table* table,
                                          const tachyon_mi355x_quotient_group* group, size_t* out) {
  static const unsigned char kAcc[32] = {};
  return guarded_report(__func__, 0, [&] {
    if (!out || !params || !qp::part_ok(params, table, group, kAcc, two_adicity(params->field))) return 0;
    if (params->field == 0) plonk::Quotient<Bn254Fr>::program_stats(*params, *table, *group, out);
    else plonk::Quotient<Bls381Fr>::program_stats(*params, *table, *group, out);
    return 1;
  });
}

size_t tachyon_mi355x_quotient_held_bytes(void) {
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  return g_quotient_held;
}

size_t tachyon_mi355x_quotient_tile_rows(void) { return plonk::kQBlock; }

size_t tachyon_mi355x_quotient_fast_slots(void) { return plonk::kQFastSlots; }

void tachyon_mi355x_quotient_last_timings(float* out_ms) {
  if (!out_ms) return;
  std::lock_guard<std::mutex> lock(g_timings_mutex);
  memcpy(out_ms, g_quotient_ms, sizeof(g_quotient_ms));
}

}  // extern "C"
