// Argument checks of tachyon_mi355x_grand_product_chains
// (include/tachyon_mi355x.h): host-only C++ with no HIP dependency, so the
// refusal rules can be compiled and run on their own.  Nothing here touches
// the GPU or dereferences a column: only the descriptor arrays are read and
// the columns' address ranges compared.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../../include/tachyon_mi355x.h"

namespace tachyon_amd::gp_validate {

inline constexpr size_t kElemBytes = 32;

inline bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

inline bool factors_ok(const tachyon_mi355x_gp_factor* f, size_t count) {
  if (count != 0 && !f) return false;
  for (size_t k = 0; k < count; ++k) {
    if (f[k].kind > 2 || !f[k].values) return false;
    if (f[k].kind == 1 && !f[k].table) return false;
  }
  return true;
}

// True when the call can run.  max_tiles: the largest tile count of one call
// (jobs x tiles per job), tile_rows the rows of a tile.
inline bool check(int field, size_t n, size_t usable_rows, const void* omega, const void* delta,
                  const tachyon_mi355x_gp_poly* polys, const size_t* chain_lens, size_t num_chains,
                  const void* blinds, void* const* out_z, size_t tile_rows, size_t max_tiles) {
  if (field != 0 && field != 2) return false;
  if (n == 0 || usable_rows >= n || n >= ((size_t)1 << 31)) return false;
  if (num_chains != 0 && !chain_lens) return false;
  size_t num_polys = 0;
  for (size_t c = 0; c < num_chains; ++c) {
    if (chain_lens[c] > max_tiles) return false;
    num_polys += chain_lens[c];
    if (num_polys > max_tiles) return false;
  }
  if (num_polys == 0) return true;
  if (!polys || !out_z) return false;
  if (num_polys * ((n + tile_rows - 1) / tile_rows) > max_tiles) return false;
  if (n - usable_rows - 1 != 0 && !blinds) return false;
  bool any_label = false;
  for (size_t i = 0; i < num_polys; ++i) {
    const tachyon_mi355x_gp_poly& p = polys[i];
    if (p.num_count == 0 && p.den_count == 0) return false;
    if (!factors_ok(p.num, p.num_count) || !factors_ok(p.den, p.den_count)) return false;
    if (!out_z[i]) return false;
    for (size_t k = 0; k < p.num_count; ++k) any_label |= p.num[k].kind == 2;
    for (size_t k = 0; k < p.den_count; ++k) any_label |= p.den[k].kind == 2;
  }
  if (any_label && (!omega || !delta)) return false;
  // an output overlaps no input column and no other output
  const size_t bytes = n * kElemBytes;
  for (size_t i = 0; i < num_polys; ++i) {
    for (size_t j = 0; j < i; ++j)
      if (overlap(out_z[i], out_z[j], bytes)) return false;
    for (size_t q = 0; q < num_polys; ++q) {
      for (int side = 0; side < 2; ++side) {
        const tachyon_mi355x_gp_factor* f = side ? polys[q].den : polys[q].num;
        const size_t cnt = side ? polys[q].den_count : polys[q].num_count;
        for (size_t k = 0; k < cnt; ++k) {
          if (overlap(out_z[i], f[k].values, bytes)) return false;
          if (f[k].kind == 1 && overlap(out_z[i], f[k].table, bytes)) return false;
        }
      }
    }
  }
  return true;
}

}  // namespace tachyon_amd::gp_validate
