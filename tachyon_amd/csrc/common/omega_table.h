// The powers of omega for a kernel whose workgroups own `block` consecutive
// rows, without an n-element column: three small tables A | B | C with
//   omega^j = A[j % block] B[(j / block) % kOmegaTabB] C[j / (block kOmegaTabB)].
// The host part takes any F with one(), operator* and canonical() and needs
// no HIP; the device part is for 8-limb Fr.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tachyon_amd {

constexpr unsigned kOmegaTabB = 256;

// Elements of the tables for rows j < n
inline size_t omega_table_size(size_t n, size_t block) {
  return block + kOmegaTabB + (n + block * kOmegaTabB - 1) / (block * kOmegaTabB);
}

template <class F>
void omega_table_fill(F* out, size_t n, size_t block, const F& omega) {
  auto powers = [](F* tab, size_t count, const F& step) {
    tab[0] = F::one();
    for (size_t k = 1; k < count; ++k) tab[k] = (tab[k - 1] * step).canonical();
    return (tab[count - 1] * step).canonical();
  };
  const F wb = powers(out, block, omega);
  const F wc = powers(out + block, kOmegaTabB, wb);
  powers(out + block + kOmegaTabB, omega_table_size(n, block) - block - kOmegaTabB, wc);
}

}  // namespace tachyon_amd

#ifdef __HIPCC__
#include "../field/fr_device.h"

namespace tachyon_amd {

// omega^(slab kBlock + thread); slab is the same in the whole workgroup
template <unsigned kBlock, class Fr>
__device__ __forceinline__ Fr omega_at(const Fr* __restrict__ wtab, unsigned thread, uint32_t slab) {
  return load_fr(wtab + thread) *
         (load_fr(wtab + kBlock + slab % kOmegaTabB) * load_fr(wtab + kBlock + kOmegaTabB + slab / kOmegaTabB));
}

}  // namespace tachyon_amd
#endif
