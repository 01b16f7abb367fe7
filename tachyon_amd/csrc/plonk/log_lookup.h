// The log-derivative lookup's prover polynomials on device-resident columns
// (DESIGN §4.9): the multiplicities m(X) and the grand sum phi(X).
//
// Reference: tachyon/zk/lookup/log_derivative_halo2/prover_impl.h:99-155
//   (ComputeMPoly / ComputeMPolys) and :186-316 (ComputeLogDerivatives,
//   CreateGrandSumPoly / CreateGrandSumPolys), base/containers/
//   container_util.h:169-185 (BinarySearchByKey), math/base/groups.h:124-143
//   (the batch inverse skips zeros), zk/base/blinder.h:33-45.
//
// A lookup has K >= 1 compressed input columns f_0 .. f_{K-1} and one
// compressed table column t, u usable rows of n.
//
// m:   the entries (i, t[i] as a canonical integer), i < u, are sorted by the
//      integer alone, ties by ascending i (fr_sort.h).  Every input value
//      f_k[j], j < u, is searched by the reference's bisection -- left = 0,
//      right = u, mid = left + (right - left) / 2, the FIRST equal hit
//      returns -- and a hit adds 1 to the counter of the hit entry's original
//      row; a miss adds nothing.  With duplicate table values the counted row
//      is the one this bisection lands on.  m[i] = counter for i < u, 0 from
//      row u on.  Launches: per lookup the sort's; then for the whole call
//      one count kernel over every (input column, row) and one kernel that
//      writes every m.
// phi: L[i] = sum_k 1 / (f_k[i] + beta) - m[i] / (t[i] + beta) for i < u, a
//      zero denominator contributing 0; phi[0] = 0, phi[i] = sum_{j<i} L[j]
//      for i < u, phi[u] = 0, rows u+1 .. n-1 the caller's blinds; the full
//      sum over all u rows is returned beside it.  Four launches for the
//      whole call, in the manner of the grand products (grand_product.h):
//   A  terms.  Rows: a workgroup owns a tile of kLlTile rows of one lookup.
//      Per row the K + 1 terms are summed as ONE fraction N / D (for a
//      nonzero denominator d with coefficient c: N <- N d + c D, D <- D d:
//      two products per input, three for the table), then Montgomery's trick
//      runs over the tile's D: q(i) = N(i) E(i) S(i) = L(i) P goes to phi's
//      own row, P (the product of the tile's D) and the sum of the q to the
//      tile's slots.  Tiles: tile_invert_kernel, one Fermat inversion per
//      tile, gives 1 / P and the tile's sum of L.
//   B  carries: one workgroup per lookup scans that lookup's tile sums,
//      kLlWalk at a time, writes every tile's carry-in and the full sum.
//   C  apply: each tile reads q(i), scans L(i) = q(i) / P, adds its carry and
//      writes phi[0..u-1] (canonical), phi[u] = 0 and the blind rows.
// L is stored (as q, in phi's rows), not recomputed in C: 32 bytes written
// and read back per row against K + 2 columns read again and 2K + 8 products.
// No kernel waits on another workgroup; nothing is ordered by atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/hip_util.h"
#include "../field/ff.h"

namespace tachyon_amd::plonk {

constexpr unsigned kLlBlock = 256;                 // threads per workgroup (4 waves)
constexpr unsigned kLlChunk = 4;                   // rows per thread
constexpr unsigned kLlTile = kLlBlock * kLlChunk;  // rows per workgroup of the grand sum: 1024
constexpr unsigned kLlWalk = kLlBlock;             // tile sums per step of the carry scan
constexpr size_t kLlMaxBlocks = (size_t)1 << 30;   // workgroups of one launch (a grid's x extent)
constexpr int kLlPhases = 5;                       // sort, count, sums A, B, C

template <class Fr>
class LogLookup {
 public:
  explicit LogLookup(hipStream_t stream) : stream_(stream) {}
  LogLookup(const LogLookup&) = delete;
  LogLookup& operator=(const LogLookup&) = delete;

  // inputs / table: n elements each, host or device
  struct Lookup {
    const Fr* const* inputs;
    size_t num_inputs;
    const Fr* table;
  };

  // The arguments are the caller's to validate (capi/log_lookup_validate.h).
  // out_m: per lookup n elements, host or device, no input; out_misses (host,
  // or null): per lookup the input values found nowhere in the table's usable
  // rows.  ms: kLlPhases times from stream events; this call sets sort and
  // count.  Synchronises the stream before it returns.
  void m_polys(size_t n, size_t u, const Lookup* lookups, size_t count, Fr* const* out_m, uint64_t* out_misses,
               float* ms);

  // m: per lookup its n multiplicities, host or device; blinds: per lookup
  // n - u - 1 elements, host or device; out_phi: per lookup n elements, host
  // or device, no input; out_totals (or null): per lookup the sum of L over
  // all u rows.  This call sets the phases A, B, C of ms.
  void grand_sums(size_t n, size_t u, const Fr& beta, const Lookup* lookups, const Fr* const* m, size_t count,
                  const Fr* blinds, Fr* const* out_phi, Fr* out_totals, float* ms);

  // Device bytes the larger of the two calls holds beyond the caller's own
  // device-resident columns and outputs, for `count` lookups of at most
  // max_inputs inputs over n rows, every column staged from the host (needs
  // a device: the sort's scratch is the sort library's to size).
  static size_t work_bytes(size_t n, size_t max_inputs, size_t count);

  hipStream_t stream() const { return stream_; }

 private:
  // device views of out[i]: in place where usable, else rows of result_
  std::vector<Fr*> outputs(Fr* const* out, size_t count, size_t n);
  void copy_out(const std::vector<Fr*>& dev, Fr* const* out, size_t count, size_t n);

  hipStream_t stream_;
  DeviceBuffer stage_, meta_, work_, result_;
  SectionPacker upload_;
};

extern template class LogLookup<Bn254Fr>;
extern template class LogLookup<Bls381Fr>;

}  // namespace tachyon_amd::plonk
