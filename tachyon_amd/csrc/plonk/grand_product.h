// Grand-product polynomials Z of the Halo2 permutation, lookup and shuffle
// arguments on device-resident columns.
//
// Reference: tachyon/zk/plonk/permutation/grand_product_argument.h:17-122
//   (CreatePoly / CreatePolySerial / CreateExcessivePoly / DoCreatePoly),
//   permutation_prover_impl.h:24-86, 216-244 (the chain over column chunks and
//   its callbacks), zk/lookup/halo2/prover_impl.h:126-138, zk/shuffle/
//   prover_impl.h:77, zk/base/blinder.h:33-45 (the blinding rows).
//
// One definition covers the three arguments.  A factor is
//   f(j) = v[j] + m t(j) + c     for rows j < n,
// t absent, a second column, or the label delta^i omega^j of permutation
// column i (computed on the device from small power tables: no n-element
// label column exists).  A poly job is a numerator and a denominator factor
// list; ratio(j) = prod num(j) / prod den(j), and 0 where the denominator is 0
// (the batch inverse's rule, math/base/groups.h:124-180).  A chain is an
// ordered list of jobs with z[0] = 1 for the first and the previous job's
// z[u] for every next one, z[j+1] = z[j] ratio(j) for j < u, and the caller's
// blinds on rows u+1 .. n-1.  One call takes several chains.
//
// Four launches for the whole call, whatever the number of chains and jobs:
//   A  ratios, in two kernels.  Rows: a workgroup owns a tile of kGpTile rows
//      of one job, forms num and den per row and, by Montgomery's trick across
//      the tile (per-thread prefix products, a prefix and a suffix scan over
//      the workgroup), q(j) = num(j) / den(j) * P for j < u into the output's
//      own rows, with P the product of the tile's denominators; it also
//      writes P and the product of the tile's numerators.  Tiles: one lane
//      per tile inverts P -- ONE Fermat inversion per tile, 64 of them side by
//      side in a wave -- and forms the product of the tile's ratios;
//   B  carries: one workgroup per chain walks that chain's tile products in
//      order through all of its jobs, kGpWalk at a time, writes every tile's
//      carry-in and the chain's final z[u];
//   C  apply: each tile scans its ratios q(j) / P, multiplies by its carry,
//      and writes z[0..u] (canonical) over them and the blind rows.
// Every input column is read once per job that uses it; there is no host
// round trip or synchronisation between the passes; no kernel waits on
// another workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/hip_util.h"
#include "../field/ff.h"

namespace tachyon_amd::plonk {

constexpr unsigned kGpBlock = 256;                   // threads per workgroup (4 waves)
constexpr unsigned kGpChunk = 4;                     // rows per thread
constexpr unsigned kGpTile = kGpBlock * kGpChunk;    // rows per workgroup: 1024
constexpr unsigned kGpWalk = kGpBlock;               // tile products per step of the carry walk
constexpr size_t kGpMaxTiles = (size_t)1 << 30;      // tiles of one call (a grid's x extent)

template <class Fr>
class GrandProduct {
 public:
  explicit GrandProduct(hipStream_t stream) : stream_(stream) {}
  GrandProduct(const GrandProduct&) = delete;
  GrandProduct& operator=(const GrandProduct&) = delete;

  enum Kind : uint32_t { kPlain = 0, kTable = 1, kLabel = 2 };
  // v[j] + m t(j) + c; values / table: n elements, host or device
  struct Factor {
    const Fr* values;
    const Fr* table;  // kTable only
    uint32_t kind;
    uint32_t label;  // kLabel: the permutation column index i
    Fr m, c;
  };
  struct Poly {
    const Factor* num;
    size_t num_count;
    const Factor* den;
    size_t den_count;
  };

  // The arguments are the caller's to validate (capi/grand_product_validate.h).
  // polys: the jobs of chain 0, then chain 1, ...; blinds: host, per poly
  // n - u - 1 elements; out_z: per poly n elements, host or device, no input;
  // out_last (host, or null): every chain's final z[u] (1 for an empty
  // chain).  ms (or null): the passes' times A, B, C from stream events.
  // Synchronises the stream before it returns.
  void run(size_t n, size_t u, const Fr& omega, const Fr& delta, const Poly* polys, const size_t* chain_lens,
           size_t num_chains, const Fr* blinds, Fr* const* out_z, Fr* out_last, float* ms);

  hipStream_t stream() const { return stream_; }

 private:
  struct Call;
  // run's four steps; copy_out synchronises the stream
  void stage(Call& c, Fr* const* out_z);
  void pack(Call& c, const Fr& omega, const Fr& delta, const Fr* blinds);
  void launch(const Call& c, PhaseClock& clock);
  void copy_out(const Call& c, Fr* const* out_z, Fr* out_last);

  hipStream_t stream_;
  DeviceBuffer stage_, meta_, prods_, result_;
  SectionPacker upload_;  // the host image of the upload in flight
};

extern template class GrandProduct<Bn254Fr>;
extern template class GrandProduct<Bls381Fr>;

}  // namespace tachyon_amd::plonk
