// The Halo2 quotient h(X) on device-resident polynomials.
//
// Reference: zk/plonk/vanishing/circuit_polynomial_builder.h:199-245 (the
// Scroll shape: for each of the P = extended_n / n parts every polynomial on
// the size-n coset zeta w_ext^i <w>, one accumulator per row folded in y over
// gates, permutation, lookups and shuffles of every circuit), vanishing_utils
// .h:183-196 (the parts interleaved, ext[j P + i] = part_i[j]), :65-112 (the
// division by X^n - 1: one constant per part), :167-180 (the coset IFFT with
// offset zeta) and vanishing_prover_impl.h:106-112 (the truncation).
//
// One kernel evaluates everything: quotient_plan.h writes each term group --
// the caller's gate graph, and the permutation, lookup and shuffle closed
// forms as fixed graphs around the caller's compressed-expression graphs -- as
// one flat program, and quotient_eval_kernel interprets it, one row per lane,
// on the accumulator in place.  The program, its constants and the column
// pointers are the same for the whole wave: they come by scalar loads from a
// read-only buffer and every branch on them is taken once per wave.  A
// program's intermediates live in kQFastSlots LDS slots per lane, laid out
// [slot][half][lane] in 16-byte cells so that one wave's access to one slot is
// contiguous; the slots beyond them spill to a [slot][row] workspace.  A
// rotated read is col[(row + r) mod n].  A last kernel per part multiplies by
// the part's 1 / (zeta^n w_ext^(n i) - 1) and scatters to ext[j P + i].
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/hip_util.h"
#include "../field/ff.h"
#include "quotient_plan.h"

namespace tachyon_amd::plonk {

constexpr unsigned kQBlock = 256;     // rows per workgroup (4 waves)
constexpr unsigned kQFastSlots = 10;  // 10 x 256 x 32 B = 80 KB of the CU's 160 KB LDS: two workgroups per CU
// timings: transforms, gates, permutation, lookups, shuffles, scatter, final inverse transform
constexpr int kQPhases = 7;

template <class Fr>
class Quotient {
 public:
  explicit Quotient(hipStream_t stream) : stream_(stream) {}
  Quotient(const Quotient&) = delete;
  Quotient& operator=(const Quotient&) = delete;

  // The arguments are the caller's to validate (quotient_plan.h part_ok /
  // h_poly_ok).  Both synchronise the stream before they return; ms: kQPhases
  // entries.
  void evaluate_part(const quotient_plan::Params& params, const quotient_plan::Table& table,
                     const quotient_plan::Group& group, void* acc, float* ms);
  void h_poly(const quotient_plan::Params& params, const quotient_plan::System& system,
              const quotient_plan::Circuit* circuits, size_t num_circuits, const Fr& zeta, const Fr& delta,
              const Fr* ext_gen, bool full, void* out, float* ms);
  // An upper bound of the device memory an h_poly call of this shape holds
  static size_t work_bytes(const quotient_plan::Params& params, const quotient_plan::System& system,
                           const quotient_plan::Circuit* circuits, size_t num_circuits);
  // out[4]: the group's lowered program -- instructions, products, column reads per row, slots needed
  static void program_stats(const quotient_plan::Params& params, const quotient_plan::Table& table,
                            const quotient_plan::Group& group, size_t* out);
  // The device memory the last h_poly call held when it returned
  size_t held_bytes() const { return held_; }

 private:
  hipStream_t stream_;
  DeviceBuffer cosets_, ext_, acc_, spill_, meta_, stage_;
  SectionPacker upload_;  // the host image of the upload in flight
  size_t held_ = 0;
};

extern template class Quotient<Bn254Fr>;
extern template class Quotient<Bls381Fr>;

}  // namespace tachyon_amd::plonk
