// The one inversion per tile of the tile-wise Montgomery trick, shared by the
// grand products (grand_product.hip) and the log-derivative grand sums
// (log_lookup.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../field/fr_device.h"

namespace tachyon_amd::plonk {

// One lane per tile: the tile's one inversion, 64 of them per wave side by
// side (a Fermat inversion is a chain of ~380 dependent products: in the row
// kernel it held a whole workgroup's registers idle behind one lane).
// dens[t] <- 1 / P_t and scaled[t] <- scaled[t] / P_t: the product of the
// tile's ratios where scaled[t] came in as the product of its numerators, the
// sum of the tile's terms where it came in as the sum of its q_r = term_r P_t.
template <class Fr>
__global__ __launch_bounds__(64) void tile_invert_kernel(Fr* __restrict__ dens, Fr* __restrict__ scaled,
                                                         uint32_t count) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  const Fr p = load_fr(dens + i);
  if (p.is_one()) return;  // a tile past the usable rows: 1 / 1, scaled as it is
  const Fr inv = p.inverse();  // a product of nonzero values
  store_fr(dens + i, inv);
  store_fr(scaled + i, load_fr(scaled + i) * inv);
}

}  // namespace tachyon_amd::plonk
