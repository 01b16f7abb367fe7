// The Halo2 lookup's permuted columns A' and S' on device-resident columns
// (DESIGN §4.10): the step between the compressed pair and the grand product Z.
//
// Reference: tachyon/zk/lookup/halo2/permute_expression_pair.h:29-142
//   (PermuteExpressionPair), lookup/halo2/prover_impl.h:74-95 (PermutePair and
//   its blinds), math/finite_fields/prime_field_fallback.h:182-184 (operator<
//   compares ToBigInt()), zk/base/blinder.h:33-45.
//
// Per lookup a compressed input column A and a compressed table column S, u
// usable rows of n.  In value order (the canonical integers):
//   A'[0..u) = A[0..u) ascending.  Row i is a first row when i = 0 or
//   A'[i] != A'[i-1], else a repeated row; R repeated rows, r(i) the rank of
//   repeated row i among them.  leftover[0..R) = the multiset S[0..u) less one
//   instance of each distinct value of A', ascending.  S'[i] = A'[i] on a
//   first row, leftover[R - 1 - r(i)] on a repeated row.  Rows u .. n-1 of A'
//   and of S' are the blinds.
// The reference walks a btree_map of the table's counts over the sorted
// inputs and hands the map's remaining values, ascending, to
// repeated_input_rows.back(); the above is what that walk leaves.
//
// Here: FrSort on both columns gives canonical sorted keys and the
// permutations (per column, as in §4.9).  Then for the whole call, every
// lookup in one launch of each kernel:
//   search  thread i < u compares key i of A with key i - 1 (a global load:
//           the neighbour may be the previous workgroup's) and writes the
//           repeated flag; a first row takes the LEFTMOST equal entry of the
//           table's sorted keys (a lower bound) and marks that position
//           consumed.  Distinct values hit distinct positions: plain byte
//           stores.  A wave's misses are one add on the lookup's counter.
//   ranks   count: per tile of kLpBlock rows the repeated and the not
//           consumed rows; carry: one workgroup per lookup scans the tile
//           counts in place, kLpBlock at a time, and leaves the totals R and
//           L; compact: leftpos[rank of a not consumed position] = position.
//   write   A'[i] = A[permA[i]]; S'[i] the same element on a first row, else
//           S[permS[leftpos[R - 1 - r(i)]]] with r(i) the tile's carry plus a
//           ballot scan of the flags; then the blind rows.  The ORIGINAL
//           Montgomery elements are read through the permutations; canonical
//           keys are never converted back.
// With misses L = R + misses > R, so every index R - 1 - r is below L and
// inside leftpos's written part; the write is skipped all the same where
// R - 1 - r >= L.  No kernel waits on another workgroup; nothing is ordered
// by atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/hip_util.h"
#include "../field/ff.h"

namespace tachyon_amd::plonk {

constexpr unsigned kLpBlock = 256;                // threads per workgroup (4 waves) = rows per scan tile
constexpr size_t kLpMaxBlocks = (size_t)1 << 30;  // workgroups of one launch (a grid's x extent)
constexpr int kLpPhases = 4;                      // sort, search, ranks, write

template <class Fr>
class LookupPermute {
 public:
  explicit LookupPermute(hipStream_t stream) : stream_(stream) {}
  LookupPermute(const LookupPermute&) = delete;
  LookupPermute& operator=(const LookupPermute&) = delete;

  // input / table: n elements each, host or device
  struct Pair {
    const Fr* input;
    const Fr* table;
  };

  // The arguments are the caller's to validate (capi/lookup_permute_validate.h).
  // blinds: per pair n - u elements for A' then n - u for S', host or device;
  // out_input / out_table: per pair n elements, host or device, no input;
  // out_misses (host, or null): per pair the distinct input values found
  // nowhere in the table's usable rows.  ms: kLpPhases times from stream
  // events.  Synchronises the stream before it returns.
  void permute_pairs(size_t n, size_t u, const Pair* pairs, size_t count, const Fr* blinds, Fr* const* out_input,
                     Fr* const* out_table, uint64_t* out_misses, float* ms);

  // Device bytes one call holds beyond the caller's own device-resident
  // columns and outputs, for `count` pairs over n rows, every column staged
  // from the host (needs a device: the sort's scratch is the sort library's
  // to size).
  static size_t work_bytes(size_t n, size_t count);

  hipStream_t stream() const { return stream_; }

 private:
  hipStream_t stream_;
  DeviceBuffer stage_, meta_, work_, result_;
  SectionPacker upload_;
};

extern template class LookupPermute<Bn254Fr>;
extern template class LookupPermute<Bls381Fr>;

}  // namespace tachyon_amd::plonk
