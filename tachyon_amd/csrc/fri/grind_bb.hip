// The proof-of-work search of Challenger::Grind for BabyBear (see grind_bb.h):
//   grind_kernel   a lane tests the candidates start + lane, + lanes, ... of a
//                  chunk in ascending order, one Poseidon2 permutation each,
//                  and stops at its first hit; the wave's smallest hit goes to
//                  one device word by atomicMin
// The host walks the range in ascending chunks, one launch each, and stops
// after the first chunk with a hit: its minimum is the range's.
#include "grind_bb.h"

#include <algorithm>
#include <type_traits>

#include "../hash/poseidon2_bb.h"

namespace tachyon_amd::fri {

namespace p2 = poseidon2_bb;

namespace {

constexpr unsigned kBlock = 256;
constexpr unsigned kWave = 64;
constexpr uint64_t kMaxLanes = uint64_t(1) << 20;  // lanes of one launch
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct GrindArgs {
  uint32_t base[16];  // the state with the input buffer laid over it
  uint32_t slot;      // where the candidate goes
  uint32_t mask;      // 2^bits - 1
  uint32_t start, end;  // canonical candidates of this launch, end <= p
};

template <int EXT>
__global__ __launch_bounds__(kBlock) void grind_kernel(const GrindArgs a, uint32_t* result) {
  const uint32_t lanes = gridDim.x * kBlock;  // end + lanes < 2^31 + 2^20: no wrap
  uint32_t found = kNone;
#pragma unroll 1
  for (uint32_t c = a.start + blockIdx.x * kBlock + threadIdx.x; c < a.end; c += lanes) {
    const uint32_t cm = bb31::to_mont(c);
    uint32_t s[16];
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) s[j] = j == a.slot ? cm : a.base[j];
    p2::permute<EXT>(s);
    if ((bb31::from_mont(s[15]) & a.mask) == 0) {
      found = c;
      break;
    }
  }
  // every lane of the wave is here: the smallest hit of the wave, then of the launch
#pragma unroll
  for (int off = kWave / 2; off > 0; off /= 2) found = min(found, (uint32_t)__shfl_xor((int)found, off, kWave));
  if (threadIdx.x % kWave == 0 && found != kNone) atomicMin(result, found);
}

}  // namespace

bool grind(DuplexChallenger& challenger, unsigned bits, uint64_t from, uint64_t to, uint32_t* witness_out,
           DeviceBuffer& scratch, hipStream_t stream, unsigned* launches) {
  if (launches) *launches = 0;
  if (!witness_out || !grind_args_ok(bits, from, to)) return false;
  require_gpu();
  GrindArgs a{};
  a.slot = challenger.grind_base(a.base);
  a.mask = (uint32_t(1) << bits) - 1;
  uint32_t* d_min = static_cast<uint32_t*>(scratch.ensure(sizeof(uint32_t)));
  TA_HIP(hipMemsetAsync(d_min, 0xFF, sizeof(uint32_t), stream));

  uint32_t found = kNone;
  unsigned count = 0;
  uint64_t chunk = grind_first_chunk(bits);
  for (uint64_t start = from; start < to && found == kNone; start += chunk, chunk = kGrindMaxChunk) {
    const uint64_t end = std::min(to, start + chunk);
    a.start = (uint32_t)start;
    a.end = (uint32_t)end;
    const unsigned blocks = ceil_div(std::min(end - start, kMaxLanes), kBlock);
    if (challenger.external() == p2::kHorizen)
      hipLaunchKernelGGL(grind_kernel<p2::kHorizen>, dim3(blocks), dim3(kBlock), 0, stream, a, d_min);
    else
      hipLaunchKernelGGL(grind_kernel<p2::kPlonky3>, dim3(blocks), dim3(kBlock), 0, stream, a, d_min);
    TA_HIP(hipGetLastError());
    ++count;
    TA_HIP(hipMemcpyAsync(&found, d_min, sizeof found, hipMemcpyDeviceToHost, stream));
    TA_HIP(hipStreamSynchronize(stream));
  }
  if (launches) *launches = count;
  if (found == kNone) return false;

  const uint32_t witness = bb31::to_mont(found);
  const DuplexChallenger before = challenger;
  if (!challenger.check_witness(bits, witness)) {  // the device and the host permutation disagree
    challenger = before;
    return false;
  }
  *witness_out = witness;
  return true;
}

}  // namespace tachyon_amd::fri
