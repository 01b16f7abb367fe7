// Dense-polynomial arithmetic over Fr on device-resident coefficient vectors:
// what a KZG opening needs between the commitments.
//
// Reference: tachyon/math/polynomials/univariate/
//   univariate_polynomial.h        Evaluate (Horner), LinearCombinationInPlace
//   univariate_dense_coefficients  operator/ by a vanishing polynomial
//                                  (FromRoots), remainder dropped
// Polynomials are coefficient vectors, lowest degree first, Montgomery form,
// of any length >= 0.
//
// Tiling: a thread owns kPolyChunk consecutive coefficients, a workgroup of
// kPolyBlock threads a tile of kPolyTile = kPolyBlock * kPolyChunk.  With
// S_j = sum_{k >= j} a_k z^(k - j) (the value at z of the suffix from j):
//   evaluation   P(z) = S_0
//   division     quotient q_{j-1} = S_j (j >= 1), remainder S_0
// and S over a tile is a per-thread Horner, a suffix scan of the affine maps
// across the wave and the workgroup (their multipliers are the known powers
// z^(kPolyChunk k), a host-built table), and the tile's carry S_(tile end).
// The per-tile values are themselves a polynomial in z^kPolyTile, so a long
// evaluation is the same kernel run again over the partials, and the carries
// of a division are the quotient of the partials by (X - z^kPolyTile), walked
// by ONE workgroup tile by tile: no kernel waits on another workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/hip_util.h"
#include "../field/ff.h"

namespace tachyon_amd::kzg {

constexpr unsigned kPolyBlock = 256;                     // threads per workgroup (4 waves)
constexpr unsigned kPolyChunk = 8;                       // coefficients per thread
constexpr unsigned kPolyTile = kPolyBlock * kPolyChunk;  // coefficients per workgroup: 2048
constexpr unsigned kPolyTableSize = 65;                  // z, then z^(kPolyChunk k) for k = 1..64

template <class Fr>
class PolyOps {
 public:
  explicit PolyOps(hipStream_t stream) : stream_(stream) {}
  PolyOps(const PolyOps&) = delete;
  PolyOps& operator=(const PolyOps&) = delete;

  // One input of a linear combination: p in device memory, 16-byte aligned
  struct Term {
    const Fr* p;
    size_t len;
    Fr c;
  };
  // One evaluation: polynomial p (device, 16-byte aligned) at z
  struct Pair {
    const Fr* p;
    size_t len;
    Fr z;
  };

  // Device views of `count` polynomials: the pointer itself where it is
  // aligned device memory, else a copy in this object's staging buffer
  // (stage_columns; valid until the next stage() call).
  void stage(const Fr* const* ptrs, const size_t* lens, size_t count, std::vector<const Fr*>* dev);

  // out[k] = sum_i c_i P_i[k] - d [k == 0] for k < out_len, one launch: every
  // P_i read once, out written once.  out: device, 16-byte aligned, not one
  // of the inputs.  Enqueued on the stream.
  void linear_combination(const Term* terms, size_t count, const Fr& d, Fr* out, size_t out_len);

  // a / prod_j (X - roots[j]) with the remainders dropped: the roots are
  // applied one after another on the device.  a: device, len coefficients;
  // out: device, max(len, nroots) - nroots coefficients, not aliasing a.
  // d_rems (device, nroots elements, or null): the remainder of each step,
  // r_j = (quotient after j roots)(roots[j]).  Enqueued on the stream.
  void divide_by_roots(const Fr* a, size_t len, const Fr* roots, size_t nroots, Fr* out, Fr* d_rems);

  // values[i] = pairs[i].p(pairs[i].z), one launch per level for the whole
  // batch; host_out receives m canonical values (synchronises the stream).
  void evaluate(const Pair* pairs, size_t m, Fr* host_out);

  void synchronize();
  hipStream_t stream() const { return stream_; }

  // z, z^(kPolyChunk k) for k = 1..64 (host arithmetic); returns z^kPolyTile
  static Fr power_table(const Fr& z, Fr* tab);

 private:
  Fr* upload(const void* host, size_t bytes, DeviceBuffer& buf);

  hipStream_t stream_;
  DeviceBuffer stage_, lc_meta_, div_meta_, ev_meta_, partials_, carries_, tmp_[2], ev_part_[2];
  // host images of the uploads still in flight (released by synchronize())
  std::vector<std::vector<unsigned char>> pending_;
};

extern template class PolyOps<Bn254Fr>;
extern template class PolyOps<Bls381Fr>;

}  // namespace tachyon_amd::kzg
