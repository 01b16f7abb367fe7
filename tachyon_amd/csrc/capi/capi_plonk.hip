// C-ABI of the Halo2 grand products (include/tachyon_mi355x.h, "PLONK grand
// products").  Reference: tachyon/zk/plonk/permutation/
// grand_product_argument.h:17-122 and its three callers; every refusal is
// decided in grand_product_validate.h before any GPU call, and a failure
// after that returns 0 with a message: this entry point never aborts.
#include "../../../include/tachyon_mi355x.h"

#include <cstring>
#include <mutex>
#include <vector>

#include "../plonk/grand_product.h"
#include "capi_guard.h"
#include "grand_product_validate.h"

using namespace tachyon_amd;

namespace {

std::mutex g_timings_mutex;
float g_last_ms[3] = {0.f, 0.f, 0.f};

struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() { TA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~OwnedStream() { (void)hipStreamDestroy(s); }
};

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

}  // extern "C"
