// Halo2 lookup: the permuted columns A' and S' (sort, search, ranks, write);
// see lookup_permute.h for the definitions.
#include "lookup_permute.h"

#include <algorithm>
#include <stdexcept>

#include "../field/fr_device.h"
#include "fr_sort.h"

namespace tachyon_amd::plonk {

namespace {

constexpr unsigned kWaves = kLpBlock / 64;

template <class Fr>
struct DevPair {
  const Fr* input;  // u rows
  const Fr* table;  // u rows
  Fr* out_input;    // n rows, 16-byte aligned
  Fr* out_table;
};

// work_ of one call: [keys of A | keys of S | perm A | perm S | leftpos | tile counts | totals | misses | repeated |
// consumed | blinds | the sort's scratch], the offsets of all but the first and the size
struct WorkLayout {
  size_t keys_s, perm_a, perm_s, left, counts, totals, miss, rep, cons, blinds, sort, size;
  WorkLayout(size_t n, size_t u, size_t count, size_t sort_scratch) {
    const size_t tiles = count * ceil_div(u, kLpBlock);
    SectionPacker lay;
    lay.add(count * u * 32);
    keys_s = lay.add(count * u * 32);
    perm_a = lay.add(count * u * sizeof(uint32_t));
    perm_s = lay.add(count * u * sizeof(uint32_t));
    left = lay.add(count * u * sizeof(uint32_t));
    counts = lay.add(2 * tiles * sizeof(uint32_t));
    totals = lay.add(2 * count * sizeof(uint32_t));
    miss = lay.add(count * sizeof(unsigned long long));
    rep = lay.add(count * u);
    cons = lay.add(count * u);
    blinds = lay.add(count * 2 * (n - u) * 32);
    sort = lay.add(sort_scratch);
    size = lay.size();
  }
};

// Exclusive count of the set flags over the workgroup in thread order: the
// flags of the threads before this one, *total those of all of them (the same
// in every thread).  lds: kWaves words; the leading barrier lets the previous
// use drain.
__device__ __forceinline__ uint32_t block_scan_flag(bool flag, uint32_t* lds, uint32_t* total) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long set = __ballot(flag);
  __syncthreads();
  if (lane == 0) lds[wave] = (uint32_t)__popcll(set);
  __syncthreads();
  uint32_t before = 0, acc = 0;
#pragma unroll
  for (unsigned i = 0; i < kWaves; ++i) {
    if (i == wave) before = acc;
    acc += lds[i];
  }
  *total = acc;
  return before + (uint32_t)__popcll(set & ((1ull << lane) - 1));
}

// The same over one word per thread
__device__ __forceinline__ uint32_t block_scan_u32(uint32_t x, uint32_t* lds, uint32_t* total) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t s = x;
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)s, d, 64);
    if (lane >= d) s += t;
  }
  __syncthreads();
  if (lane == 63) lds[wave] = s;
  __syncthreads();
  uint32_t before = 0, acc = 0;
#pragma unroll
  for (unsigned i = 0; i < kWaves; ++i) {
    if (i == wave) before = acc;
    acc += lds[i];
  }
  *total = acc;
  return before + s - x;
}

// Flag and search.  grid: blocks_per_job x lookups, flat; thread i < u owns
// sorted input key i of its lookup.  repeated[i] <- key i == key i - 1 (the
// neighbour is read from memory: it may be the previous workgroup's last
// key).  A first row bisects the table's sorted keys for the leftmost entry
// not below its key; an equal one is marked consumed, anything else is a miss.
template <class Fr>
__global__ __launch_bounds__(kLpBlock) void lp_search_kernel(const Fr* __restrict__ keys_a,
                                                             const Fr* __restrict__ keys_s, uint32_t u,
                                                             uint32_t blocks_per_job,
                                                             unsigned char* __restrict__ repeated,
                                                             unsigned char* __restrict__ consumed,
                                                             unsigned long long* __restrict__ misses) {
  const uint32_t lookup = blockIdx.x / blocks_per_job;
  const uint32_t i = (blockIdx.x - lookup * blocks_per_job) * kLpBlock + threadIdx.x;
  const size_t first = (size_t)lookup * u;
  bool missed = false;
  if (i < u) {
    const Fr x = load_fr(keys_a + first + i);
    const bool rep = i != 0 && compare_key(keys_a + first + i - 1, x) == 0;
    repeated[first + i] = rep;
    if (!rep) {
      const Fr* keys = keys_s + first;
      uint32_t left = 0, right = u;
      while (left < right) {
        const uint32_t mid = left + (right - left) / 2;
        if (compare_key(keys + mid, x) < 0) left = mid + 1;
        else right = mid;
      }
      if (left < u && compare_key(keys + left, x) == 0) consumed[first + left] = 1;
      else missed = true;
    }
  }
  const unsigned long long m = __ballot(missed);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(misses + lookup, (unsigned long long)__popcll(m));
}

// Ranks, count.  grid: tiles_per_job x lookups, flat.  counts[0][tile] <- the
// tile's repeated rows, counts[1][tile] <- its rows not consumed; counts[1]
// starts `tiles` words after counts[0].
__global__ __launch_bounds__(kLpBlock) void lp_count_kernel(const unsigned char* __restrict__ repeated,
                                                            const unsigned char* __restrict__ consumed, uint32_t u,
                                                            uint32_t tiles_per_job, uint32_t* __restrict__ counts) {
  __shared__ uint32_t lds[kWaves];
  const uint32_t lookup = blockIdx.x / tiles_per_job;
  const uint32_t i = (blockIdx.x - lookup * tiles_per_job) * kLpBlock + threadIdx.x;
  const size_t at = (size_t)lookup * u + i, tiles = (size_t)gridDim.x;
  uint32_t reps, frees;
  block_scan_flag(i < u && repeated[at], lds, &reps);
  block_scan_flag(i < u && !consumed[at], lds, &frees);
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = reps;
    counts[tiles + blockIdx.x] = frees;
  }
}

// Ranks, carry.  grid: lookups x 2 (blockIdx.y: repeated, not consumed).  One
// workgroup scans one lookup's tile counts in place, kLpBlock at a time, the
// carry kept in a register from one step to the next; totals[2 lookup + y] <-
// the sum: R and L.
__global__ __launch_bounds__(kLpBlock) void lp_carry_kernel(uint32_t* __restrict__ counts, uint32_t tiles_per_job,
                                                            uint32_t* __restrict__ totals) {
  __shared__ uint32_t lds[kWaves];
  uint32_t* mine = counts + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * tiles_per_job;
  uint32_t carry = 0;
  for (uint32_t i0 = 0; i0 < tiles_per_job; i0 += kLpBlock) {
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t x = i < tiles_per_job ? mine[i] : 0;
    uint32_t total;
    const uint32_t e = block_scan_u32(x, lds, &total);
    if (i < tiles_per_job) mine[i] = carry + e;
    carry += total;
  }
  if (threadIdx.x == 0) totals[2 * blockIdx.x + blockIdx.y] = carry;
}

// Ranks, compact.  grid: tiles_per_job x lookups, flat.  leftpos[k] <- the
// k-th position of the table's sorted keys that no first row consumed.
__global__ __launch_bounds__(kLpBlock) void lp_compact_kernel(const unsigned char* __restrict__ consumed, uint32_t u,
                                                              uint32_t tiles_per_job,
                                                              const uint32_t* __restrict__ carries,
                                                              uint32_t* __restrict__ leftpos) {
  __shared__ uint32_t lds[kWaves];
  const uint32_t lookup = blockIdx.x / tiles_per_job;
  const uint32_t i = (blockIdx.x - lookup * tiles_per_job) * kLpBlock + threadIdx.x;
  const size_t first = (size_t)lookup * u;
  const bool free_row = i < u && !consumed[first + i];
  uint32_t unused;
  const uint32_t k = carries[blockIdx.x] + block_scan_flag(free_row, lds, &unused);
  if (free_row) leftpos[first + k] = i;  // k < the lookup's L <= u
}

// Write.  grid: blocks_per_job x lookups, flat, over all n rows.  Row i < u:
// A'[i] <- A[permA[i]]; S'[i] <- the same element on a first row, else
// S[permS[leftpos[R - 1 - r]]], r = the tile's carry + the repeated rows
// before i in the tile; skipped where R - 1 - r >= L (which a lookup with or
// without misses never reaches, see lookup_permute.h).  Row i >= u: the
// blinds, A's n - u before S's.  Consecutive lanes write consecutive
// elements; the reads through the permutations go where the sort sent them.
template <class Fr>
__global__ __launch_bounds__(kLpBlock) void lp_write_kernel(const DevPair<Fr>* __restrict__ pairs,
                                                            const uint32_t* __restrict__ perm_a,
                                                            const uint32_t* __restrict__ perm_s,
                                                            const unsigned char* __restrict__ repeated,
                                                            const uint32_t* __restrict__ carries,
                                                            const uint32_t* __restrict__ totals,
                                                            const uint32_t* __restrict__ leftpos,
                                                            const Fr* __restrict__ blinds, uint32_t n, uint32_t u,
                                                            uint32_t blocks_per_job, uint32_t tiles_per_job) {
  __shared__ uint32_t lds[kWaves];
  const uint32_t lookup = blockIdx.x / blocks_per_job, tile = blockIdx.x - lookup * blocks_per_job;
  const uint32_t i = tile * kLpBlock + threadIdx.x;
  const DevPair<Fr> pair = pairs[lookup];
  const size_t first = (size_t)lookup * u;
  if (tile < tiles_per_job) {  // a tile with rows < u (uniform over the workgroup: the scan has barriers)
    const bool rep = i < u && repeated[first + i];
    uint32_t unused;
    const uint32_t r = carries[(size_t)lookup * tiles_per_job + tile] + block_scan_flag(rep, lds, &unused);
    if (i < u) {
      const Fr a = load_fr(pair.input + perm_a[first + i]);
      store_fr(pair.out_input + i, a);
      if (!rep) {
        store_fr(pair.out_table + i, a);
      } else {
        const uint32_t R = totals[2 * lookup], L = totals[2 * lookup + 1];
        const uint32_t k = R - 1 - r;  // r < R
        if (k < L) store_fr(pair.out_table + i, load_fr(pair.table + perm_s[first + leftpos[first + k]]));
      }
    }
  }
  if (i >= u && i < n) {
    const Fr* bl = blinds + (size_t)lookup * 2 * (n - u);
    store_fr(pair.out_input + i, load_fr(bl + (i - u)));
    store_fr(pair.out_table + i, load_fr(bl + (n - u) + (i - u)));
  }
}

}  // namespace

template <class Fr>
void LookupPermute<Fr>::permute_pairs(size_t n, size_t u, const Pair* pairs, size_t count, const Fr* blinds,
                                      Fr* const* out_input, Fr* const* out_table, uint64_t* out_misses, float* ms) {
  for (int p = 0; p < kLpPhases; ++p) ms[p] = 0.f;
  if (!count) return;
  const size_t bpn = ceil_div(n, kLpBlock), tpj = ceil_div(u, kLpBlock), tiles = count * tpj;
  drained_on_throw(stream_, [&] {
    if (count * bpn > kLpMaxBlocks) throw std::runtime_error("lookup permute: too many rows for one call");
    // device views: every pair's input, then its table (u rows of each)
    std::vector<const Fr*> cols;
    for (size_t l = 0; l < count; ++l) {
      cols.push_back(pairs[l].input);
      cols.push_back(pairs[l].table);
    }
    const std::vector<size_t> lens(cols.size(), u);
    const std::vector<const Fr*> dev = stage_columns(cols.data(), lens.data(), cols.size(), stage_, stream_);
    // device views of the outputs: in place where usable, else rows of result_
    std::vector<Fr*> want(2 * count), outs(2 * count);
    size_t held = 0;
    for (size_t l = 0; l < count; ++l) want[2 * l] = out_input[l], want[2 * l + 1] = out_table[l];
    for (Fr* p : want) held += usable_in_place(p) ? 0 : 1;
    Fr* res = held ? static_cast<Fr*>(result_.ensure(held * n * sizeof(Fr))) : nullptr;
    for (size_t i = 0, k = 0; i < 2 * count; ++i) outs[i] = usable_in_place(want[i]) ? want[i] : res + n * k++;

    const auto scratch = FrSort<Fr>::scratch(u, stream_);
    const size_t blind_elems = count * 2 * (n - u);
    const WorkLayout lay(n, u, count, scratch.total);
    unsigned char* work = static_cast<unsigned char*>(work_.ensure(lay.size));
    Fr* keys_a = reinterpret_cast<Fr*>(work);
    Fr* keys_s = reinterpret_cast<Fr*>(work + lay.keys_s);
    uint32_t* perm_a = reinterpret_cast<uint32_t*>(work + lay.perm_a);
    uint32_t* perm_s = reinterpret_cast<uint32_t*>(work + lay.perm_s);
    uint32_t* leftpos = reinterpret_cast<uint32_t*>(work + lay.left);
    uint32_t* counts = reinterpret_cast<uint32_t*>(work + lay.counts);
    uint32_t* totals = reinterpret_cast<uint32_t*>(work + lay.totals);
    auto* misses = reinterpret_cast<unsigned long long*>(work + lay.miss);
    unsigned char* repeated = work + lay.rep;
    unsigned char* consumed = work + lay.cons;
    Fr* d_blinds = reinterpret_cast<Fr*>(work + lay.blinds);
    TA_HIP(hipMemcpyAsync(d_blinds, blinds, blind_elems * sizeof(Fr), hipMemcpyDefault, stream_));

    // the upload: the pairs
    upload_.reset();
    upload_.add(count * sizeof(DevPair<Fr>));
    unsigned char* meta = upload_.image();
    auto* h_pairs = reinterpret_cast<DevPair<Fr>*>(meta);
    for (size_t l = 0; l < count; ++l) h_pairs[l] = {dev[2 * l], dev[2 * l + 1], outs[2 * l], outs[2 * l + 1]};
    const auto* d_pairs = reinterpret_cast<const DevPair<Fr>*>(upload_image(upload_, meta_, stream_));

    PhaseClock clock(stream_);
    clock.begin(0);
    for (size_t l = 0; l < count; ++l) {
      FrSort<Fr>::run(dev[2 * l], (uint32_t)u, perm_a + l * u, keys_a + l * u, work + lay.sort, scratch, stream_);
      FrSort<Fr>::run(dev[2 * l + 1], (uint32_t)u, perm_s + l * u, keys_s + l * u, work + lay.sort, scratch, stream_);
    }
    clock.end();
    clock.begin(1);
    TA_HIP(hipMemsetAsync(consumed, 0, count * u, stream_));
    TA_HIP(hipMemsetAsync(misses, 0, count * sizeof(unsigned long long), stream_));
    hipLaunchKernelGGL(lp_search_kernel<Fr>, dim3((unsigned)tiles), dim3(kLpBlock), 0, stream_, keys_a, keys_s,
                       (uint32_t)u, (uint32_t)tpj, repeated, consumed, misses);
    clock.end();
    clock.begin(2);
    hipLaunchKernelGGL(lp_count_kernel, dim3((unsigned)tiles), dim3(kLpBlock), 0, stream_, repeated, consumed,
                       (uint32_t)u, (uint32_t)tpj, counts);
    hipLaunchKernelGGL(lp_carry_kernel, dim3((unsigned)count, 2), dim3(kLpBlock), 0, stream_, counts, (uint32_t)tpj,
                       totals);
    hipLaunchKernelGGL(lp_compact_kernel, dim3((unsigned)tiles), dim3(kLpBlock), 0, stream_, consumed, (uint32_t)u,
                       (uint32_t)tpj, counts + tiles, leftpos);
    clock.end();
    clock.begin(3);
    hipLaunchKernelGGL(lp_write_kernel<Fr>, dim3((unsigned)(count * bpn)), dim3(kLpBlock), 0, stream_, d_pairs, perm_a,
                       perm_s, repeated, counts, totals, leftpos, d_blinds, (uint32_t)n, (uint32_t)u, (uint32_t)bpn,
                       (uint32_t)tpj);
    clock.end();
    TA_HIP(hipGetLastError());
    for (size_t i = 0; i < 2 * count; ++i)
      if (outs[i] != want[i]) TA_HIP(hipMemcpyAsync(want[i], outs[i], n * sizeof(Fr), hipMemcpyDefault, stream_));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the miss counters");
    if (out_misses)
      TA_HIP(hipMemcpyAsync(out_misses, misses, count * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
    TA_HIP(hipStreamSynchronize(stream_));
    clock.sum(ms, kLpPhases);
  });
}

template <class Fr>
size_t LookupPermute<Fr>::work_bytes(size_t n, size_t count) {
  if (!count || n < 2) return 0;
  // Both columns staged (u rows) and both outputs held (n rows), work_ as permute_pairs lays it out, the pairs.
  // The call has no u: u = n - 1 is the largest of all, since a usable row costs work_ more (two keys, three
  // words, two flags, the sort's scratch) than the two blinds of a row that is not
  const size_t u = n - 1;
  return 2 * count * (u + n) * sizeof(Fr) + WorkLayout(n, u, count, FrSort<Fr>::scratch(u, nullptr).total).size +
         align16(count * sizeof(DevPair<Fr>));
}

template class LookupPermute<Bn254Fr>;
template class LookupPermute<Bls381Fr>;

}  // namespace tachyon_amd::plonk
