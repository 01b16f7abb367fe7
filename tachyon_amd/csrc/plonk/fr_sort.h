// Stable sort of 8-limb scalar-field elements by their canonical integer value
// (DESIGN §4.9): the order of base::StableSort over (row, ToBigInt()) pairs
// compared by the integer alone -- ascending value, ties by ascending row.
//
// The elements come in Montgomery form.  One kernel converts them to canonical
// limbs (one Montgomery reduction each); then four passes, least significant
// 64-bit limb first, each a gather of that limb through the current
// permutation and a stable rocprim::radix_sort_pairs of (limb, row).  A stable
// pass keeps the order of the passes before it among equal limbs, so after the
// most significant one the rows are in lexicographic order of (limb 3, limb 2,
// limb 1, limb 0, row): the integer order with ties by row.  The top limb's
// pass sorts only the bits the modulus has there.  A last gather writes the
// sorted canonical keys.  Nothing depends on thread timing: every step is a
// deterministic function of its input.
//
// Four passes of 64 bits, not one of 256: rocPRIM's largest radix key is 128
// bits and its sorts move the key with every pass, so a wider key moves more
// bytes per pass than the 12 bytes of (limb, row) here while the number of
// 8-bit digit passes (32) stays what it is.
#pragma once
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <cstddef>
#include <cstdint>

#include "../common/hip_util.h"
#include "../common/sections.h"
#include "../field/ff.h"
#include "../field/fr_device.h"

namespace tachyon_amd::plonk {

constexpr unsigned kFrSortBlock = 256;

// canon[i] <- the canonical integer of in[i] (as limbs); perm[i] <- i
template <class Fr>
__global__ __launch_bounds__(kFrSortBlock) void fr_sort_canon_kernel(const Fr* __restrict__ in, uint32_t count,
                                                                     Fr* __restrict__ canon,
                                                                     uint32_t* __restrict__ perm) {
  const uint32_t i = blockIdx.x * kFrSortBlock + threadIdx.x;
  if (i >= count) return;
  store_fr(canon + i, load_fr(in + i).from_mont());
  perm[i] = i;
}

// keys[i] <- the 64-bit limb `limb` of canon[perm[i]]
template <class Fr>
__global__ __launch_bounds__(kFrSortBlock) void fr_sort_limb_kernel(const Fr* __restrict__ canon,
                                                                    const uint32_t* __restrict__ perm,
                                                                    uint32_t count, uint32_t limb,
                                                                    uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * kFrSortBlock + threadIdx.x;
  if (i >= count) return;
  const uint2 w = reinterpret_cast<const uint2*>(canon + perm[i])[limb];
  keys[i] = (uint64_t)w.x | (uint64_t)w.y << 32;
}

// sorted[i] <- canon[perm[i]]
template <class Fr>
__global__ __launch_bounds__(kFrSortBlock) void fr_sort_gather_kernel(const Fr* __restrict__ canon,
                                                                      const uint32_t* __restrict__ perm,
                                                                      uint32_t count, Fr* __restrict__ sorted) {
  const uint32_t i = blockIdx.x * kFrSortBlock + threadIdx.x;
  if (i >= count) return;
  store_fr(sorted + i, load_fr(canon + perm[i]));
}

template <class Fr>
struct FrSort {
  static_assert(sizeof(Fr) == 32, "8-limb scalar fields");
  static constexpr unsigned kTopBits = Fr::Config::kModulusBits - 192;  // of the most significant 64-bit limb

  // The scratch of one sort of `count` elements: [canon | keys in | keys out | perm alt | rocPRIM's]
  struct Scratch {
    size_t keys_in, keys_out, alt, prim, prim_bytes, total;
  };
  static Scratch scratch(size_t count, hipStream_t stream) {
    Scratch s{};
    SectionPacker p;
    p.add(count * sizeof(Fr));
    s.keys_in = p.add(count * sizeof(uint64_t));
    s.keys_out = p.add(count * sizeof(uint64_t));
    s.alt = p.add(count * sizeof(uint32_t));
    TA_HIP(rocprim::radix_sort_pairs(nullptr, s.prim_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                     (uint32_t*)nullptr, (uint32_t*)nullptr, count, 0u, 64u, stream));
    s.prim = p.add(s.prim_bytes);
    s.total = align16(p.size());
    return s;
  }

  // in: count Montgomery elements (device, 16-byte aligned).  perm[i] <- the
  // row of the i-th smallest, sorted[i] <- its canonical limbs.  work: device,
  // 16-byte aligned, scratch(count).total bytes.  Enqueues on `stream` only.
  static void run(const Fr* in, uint32_t count, uint32_t* perm, Fr* sorted, unsigned char* work, const Scratch& s,
                  hipStream_t stream) {
    if (!count) return;
    Fr* canon = reinterpret_cast<Fr*>(work);
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(work + s.keys_in);
    uint64_t* keys_out = reinterpret_cast<uint64_t*>(work + s.keys_out);
    uint32_t* alt = reinterpret_cast<uint32_t*>(work + s.alt);
    const dim3 grid(ceil_div(count, kFrSortBlock)), block(kFrSortBlock);
    hipLaunchKernelGGL(fr_sort_canon_kernel<Fr>, grid, block, 0, stream, in, count, canon, perm);
    uint32_t *from = perm, *to = alt;  // four passes: the last one lands in perm
    for (uint32_t limb = 0; limb < 4; ++limb) {
      hipLaunchKernelGGL(fr_sort_limb_kernel<Fr>, grid, block, 0, stream, canon, from, count, limb, keys_in);
      size_t bytes = s.prim_bytes;
      TA_HIP(rocprim::radix_sort_pairs(work + s.prim, bytes, keys_in, keys_out, from, to, (size_t)count, 0u,
                                       limb == 3 ? kTopBits : 64u, stream));
      uint32_t* t = from;
      from = to;
      to = t;
    }
    hipLaunchKernelGGL(fr_sort_gather_kernel<Fr>, grid, block, 0, stream, canon, perm, count, sorted);
    TA_HIP(hipGetLastError());
  }
};

}  // namespace tachyon_amd::plonk
