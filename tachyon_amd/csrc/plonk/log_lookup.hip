// Log-derivative lookup: multiplicities (sort, search and count) and grand
// sums (terms, carries, apply); see log_lookup.h for the definitions.
#include "log_lookup.h"

#include <algorithm>
#include <stdexcept>

#include "../field/fr_device.h"
#include "fr_sort.h"
#include "tile_invert.h"

namespace tachyon_amd::plonk {

namespace {

constexpr unsigned kWaves = kLlBlock / 64;

template <class Fr>
struct DevCountJob {
  const Fr* input;  // u rows
  uint32_t lookup;
  uint32_t pad;
};

template <class Fr>
struct DevSumJob {
  const Fr* table;
  const Fr* m;
  Fr* phi;              // n rows, 16-byte aligned
  uint32_t begin, end;  // its inputs in the call's pointer list
};

// Search and count.  grid: blocks_per_job x jobs, flat; a job is one input
// column of one lookup, a thread one of its rows j < u.  BinarySearchByKey
// over the lookup's sorted keys; a hit adds 1 to the counter of the hit
// entry's original row.  Where every hit of a wave is on one row (a column of
// one repeated value) one lane adds the wave's count: 64 times fewer adds on
// that counter.  The misses of a wave go to the lookup's miss counter as one
// add.
template <class Fr>
__global__ __launch_bounds__(kLlBlock) void ll_count_kernel(const DevCountJob<Fr>* __restrict__ jobs,
                                                            const Fr* __restrict__ sorted,
                                                            const uint32_t* __restrict__ perm, uint32_t u,
                                                            uint32_t blocks_per_job, uint32_t* __restrict__ counters,
                                                            unsigned long long* __restrict__ misses) {
  const uint32_t job = blockIdx.x / blocks_per_job;
  const uint32_t j = (blockIdx.x - job * blocks_per_job) * kLlBlock + threadIdx.x;
  const DevCountJob<Fr> jb = jobs[job];
  const size_t first = (size_t)jb.lookup * u;
  const bool active = j < u;
  bool found = false;
  uint32_t row = 0;
  if (active) {
    const Fr x = load_fr(jb.input + j).from_mont();
    const Fr* keys = sorted + first;
    uint32_t left = 0, right = u;
    while (left < right) {
      const uint32_t mid = left + (right - left) / 2;
      const int c = compare_key(keys + mid, x);
      if (c < 0) {
        left = mid + 1;
      } else if (c > 0) {
        right = mid;
      } else {
        found = true;
        row = perm[first + mid];
        break;
      }
    }
  }
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long hits = __ballot(found);
  if (hits) {
    const int lead = __ffsll((long long)hits) - 1;
    const uint32_t lead_row = (uint32_t)__shfl((int)row, lead, 64);
    const unsigned long long same = __ballot(found && row == lead_row);
    if (same == hits) {
      if ((int)lane == lead) atomicAdd(counters + first + lead_row, (uint32_t)__popcll(hits));
    } else if (found) {
      atomicAdd(counters + first + row, 1u);
    }
  }
  const unsigned long long missed = __ballot(active && !found);
  if (missed && lane == 0) atomicAdd(misses + jb.lookup, (unsigned long long)__popcll(missed));
}

// m[i] <- the counter as a field element for i < u, 0 for u <= i < n.
// grid: blocks_per_job x lookups, flat.
template <class Fr>
__global__ __launch_bounds__(kLlBlock) void ll_m_kernel(Fr* const* __restrict__ outs,
                                                        const uint32_t* __restrict__ counters, uint32_t n, uint32_t u,
                                                        uint32_t blocks_per_job) {
  const uint32_t lookup = blockIdx.x / blocks_per_job;
  const uint32_t i = (blockIdx.x - lookup * blocks_per_job) * kLlBlock + threadIdx.x;
  if (i >= n) return;
  Fr x = Fr::zero();
  if (i < u) {
    x.v[0] = counters[(size_t)lookup * u + i];
    x = x.to_mont().canonical();
  }
  store_fr(outs[lookup] + i, x);
}

// One more term c / d into the fraction num / den; a zero d contributes 0
template <class Fr>
__device__ __forceinline__ void add_inverse(Fr& num, Fr& den, const Fr& d) {
  if (d.is_zero()) return;
  num = num * d + den;
  den = den * d;
}

// Pass A, rows.  grid: tiles_per_job x lookups, flat.  Thread t of tile T
// owns the rows T kLlTile + k kLlBlock + t (consecutive lanes read
// consecutive elements; nothing here depends on the order of a tile's rows).
// Per row L = num / den with den the product of the row's nonzero
// denominators (never 0).  Montgomery's trick across the tile without its
// inversion: with P the product of the tile's den and E_r, S_r the products
// of those before and after row r, q_r = num_r E_r S_r = L_r P goes to phi's
// own row, P to dens[tile] and the sum of the q_r to sums[tile].
template <class Fr>
__global__ __launch_bounds__(kLlBlock) void ll_terms_kernel(const DevSumJob<Fr>* __restrict__ jobs,
                                                            const Fr* const* __restrict__ inputs, const Fr beta,
                                                            uint32_t u, uint32_t tiles_per_job, Fr* __restrict__ sums,
                                                            Fr* __restrict__ dens) {
  __shared__ Fr lds[kWaves];
  const uint32_t lookup = blockIdx.x / tiles_per_job, tile = blockIdx.x - lookup * tiles_per_job;
  const uint32_t base = tile * kLlTile;
  if (base >= u) {  // no row of the sum in this tile
    if (threadIdx.x == 0) {
      store_fr(sums + blockIdx.x, Fr::zero());
      store_fr(dens + blockIdx.x, Fr::one());
    }
    return;
  }
  const DevSumJob<Fr> job = jobs[lookup];
  Fr num[kLlChunk], den[kLlChunk];
#pragma unroll
  for (unsigned k = 0; k < kLlChunk; ++k) num[k] = Fr::zero(), den[k] = Fr::one();
  for (uint32_t f = job.begin; f < job.end; ++f) {
    const Fr* col = inputs[f];
#pragma unroll
    for (unsigned k = 0; k < kLlChunk; ++k) {
      const uint32_t j = base + k * kLlBlock + threadIdx.x;
      if (j < u) add_inverse(num[k], den[k], load_fr(col + j) + beta);
    }
  }
#pragma unroll
  for (unsigned k = 0; k < kLlChunk; ++k) {
    const uint32_t j = base + k * kLlBlock + threadIdx.x;
    if (j >= u) continue;
    const Fr d = load_fr(job.table + j) + beta;
    if (d.is_zero()) continue;  // the term m / 0 is forced to 0
    num[k] = num[k] * d - load_fr(job.m + j) * den[k];
    den[k] = den[k] * d;
  }

  // pre[k]: this thread's den[0..k]
  Fr pre[kLlChunk], run = Fr::one();
#pragma unroll
  for (unsigned k = 0; k < kLlChunk; ++k) {
    run = run * den[k];
    pre[k] = run;
  }
  Fr total, unused;
  const Fr before = block_scan_mul<Fr, kLlBlock, false>(run, lds, &total);
  Fr after = block_scan_mul<Fr, kLlBlock, true>(run, lds, &unused);  // then also this thread's den[k+1..]
  Fr qsum = Fr::zero();
#pragma unroll
  for (int k = (int)kLlChunk - 1; k >= 0; --k) {
    const Fr q = num[k] * ((k ? before * pre[k ? k - 1 : 0] : before) * after);  // rows >= u: 0
    after = after * den[k];
    qsum = qsum + q;
    const uint32_t j = base + k * kLlBlock + threadIdx.x;
    if (j < u) store_fr(job.phi + j, q);
  }
  Fr qtotal;
  block_scan_add<Fr, kLlBlock>(qsum, lds, &qtotal);
  if (threadIdx.x == 0) {
    store_fr(sums + blockIdx.x, qtotal);
    store_fr(dens + blockIdx.x, total);
  }
}

// Pass B.  One workgroup per lookup: an exclusive scan of the lookup's tile
// sums, kLlWalk at a time, the carry kept in registers from one step to the
// next; totals[lookup] <- the sum of L over all u rows.
template <class Fr>
__global__ __launch_bounds__(kLlBlock) void ll_carry_kernel(const Fr* __restrict__ sums, Fr* __restrict__ carries,
                                                            Fr* __restrict__ totals, uint32_t tiles_per_job) {
  __shared__ Fr lds[kWaves];
  const size_t first = (size_t)blockIdx.x * tiles_per_job;
  Fr carry = Fr::zero();
  for (uint32_t i0 = 0; i0 < tiles_per_job; i0 += kLlWalk) {
    const uint32_t i = i0 + threadIdx.x;
    const Fr x = i < tiles_per_job ? load_fr(sums + first + i) : Fr::zero();
    Fr total;
    const Fr e = block_scan_add<Fr, kLlBlock>(x, lds, &total);
    if (i < tiles_per_job) store_fr(carries + first + i, carry + e);
    carry = carry + total;
  }
  if (threadIdx.x == 0) store_fr(totals + blockIdx.x, carry.canonical());
}

// Pass C.  Thread t of tile T owns the rows T kLlTile + t kLlChunk + k: it
// reads its q_r (L_r = q_r invs[tile]), then writes phi over the same rows:
// the sum of the L before the row for rows < u, 0 at row u, the blinds after.
template <class Fr>
__global__ __launch_bounds__(kLlBlock) void ll_apply_kernel(const DevSumJob<Fr>* __restrict__ jobs,
                                                            const Fr* __restrict__ carries,
                                                            const Fr* __restrict__ invs,
                                                            const Fr* __restrict__ blinds, uint32_t n, uint32_t u,
                                                            uint32_t tiles_per_job) {
  __shared__ Fr lds[kWaves];
  const uint32_t lookup = blockIdx.x / tiles_per_job, tile = blockIdx.x - lookup * tiles_per_job;
  const uint32_t base = tile * kLlTile, j0 = base + threadIdx.x * kLlChunk;
  Fr* phi = jobs[lookup].phi;
  const Fr* bl = blinds + (size_t)lookup * (n - u - 1);
  if (base > u) {  // blind rows only
#pragma unroll
    for (unsigned k = 0; k < kLlChunk; ++k)
      if (j0 + k < n) store_fr(phi + j0 + k, load_fr(bl + (j0 + k - u - 1)));
    return;
  }
  const Fr inv = load_fr(invs + blockIdx.x);
  Fr r[kLlChunk], p = Fr::zero();
#pragma unroll
  for (unsigned k = 0; k < kLlChunk; ++k) {
    r[k] = j0 + k < u ? load_fr(phi + j0 + k) * inv : Fr::zero();
    p = p + r[k];
  }
  Fr total;
  Fr acc = load_fr(carries + blockIdx.x) + block_scan_add<Fr, kLlBlock>(p, lds, &total);
#pragma unroll
  for (unsigned k = 0; k < kLlChunk; ++k) {
    const uint32_t j = j0 + k;
    if (j < u) store_fr(phi + j, acc.canonical());
    else if (j == u) store_fr(phi + j, Fr::zero());
    else if (j < n) store_fr(phi + j, load_fr(bl + (j - u - 1)));
    acc = acc + r[k];
  }
}

template <class Fr>
size_t total_inputs(const typename LogLookup<Fr>::Lookup* lookups, size_t count) {
  size_t total = 0;
  for (size_t l = 0; l < count; ++l) total += lookups[l].num_inputs;
  return total;
}

}  // namespace

template <class Fr>
std::vector<Fr*> LogLookup<Fr>::outputs(Fr* const* out, size_t count, size_t n) {
  size_t held = 0;
  for (size_t i = 0; i < count; ++i) held += usable_in_place(out[i]) ? 0 : 1;
  Fr* res = held ? static_cast<Fr*>(result_.ensure(held * n * sizeof(Fr))) : nullptr;
  std::vector<Fr*> dev(count);
  for (size_t i = 0, k = 0; i < count; ++i) dev[i] = usable_in_place(out[i]) ? out[i] : res + n * k++;
  return dev;
}

template <class Fr>
void LogLookup<Fr>::copy_out(const std::vector<Fr*>& dev, Fr* const* out, size_t count, size_t n) {
  for (size_t i = 0; i < count; ++i)
    if (dev[i] != out[i]) TA_HIP(hipMemcpyAsync(out[i], dev[i], n * sizeof(Fr), hipMemcpyDefault, stream_));
}

template <class Fr>
void LogLookup<Fr>::m_polys(size_t n, size_t u, const Lookup* lookups, size_t count, Fr* const* out_m,
                            uint64_t* out_misses, float* ms) {
  ms[0] = ms[1] = 0.f;
  if (!count) return;
  const size_t num_jobs = total_inputs<Fr>(lookups, count);
  const size_t bpj = ceil_div(u, kLlBlock), bpm = ceil_div(n, kLlBlock);
  drained_on_throw(stream_, [&] {
    if (num_jobs * bpj > kLlMaxBlocks || count * bpm > kLlMaxBlocks)
      throw std::runtime_error("log lookup: too many rows for one call");
    for (size_t l = 0; l < count; ++l)  // the counters are 32 bits wide
      if (lookups[l].num_inputs > UINT32_MAX / u) throw std::runtime_error("log lookup: too many inputs for one lookup");
    // device views: every lookup's inputs, then its table (u rows of each)
    std::vector<const Fr*> cols;
    for (size_t l = 0; l < count; ++l) {
      cols.insert(cols.end(), lookups[l].inputs, lookups[l].inputs + lookups[l].num_inputs);
      cols.push_back(lookups[l].table);
    }
    const std::vector<size_t> lens(cols.size(), u);
    const std::vector<const Fr*> dev = stage_columns(cols.data(), lens.data(), cols.size(), stage_, stream_);
    const std::vector<Fr*> outs = outputs(out_m, count, n);

    // work_: [sorted keys | permutations | counters | misses | the sort's scratch]
    const auto scratch = FrSort<Fr>::scratch(u, stream_);
    SectionPacker lay;
    lay.add(count * u * sizeof(Fr));
    const size_t off_perm = lay.add(count * u * sizeof(uint32_t));
    const size_t off_cnt = lay.add(count * u * sizeof(uint32_t));
    const size_t off_miss = lay.add(count * sizeof(unsigned long long));
    const size_t off_sort = lay.add(scratch.total);
    unsigned char* work = static_cast<unsigned char*>(work_.ensure(lay.size()));
    Fr* sorted = reinterpret_cast<Fr*>(work);
    uint32_t* perm = reinterpret_cast<uint32_t*>(work + off_perm);
    uint32_t* counters = reinterpret_cast<uint32_t*>(work + off_cnt);
    auto* misses = reinterpret_cast<unsigned long long*>(work + off_miss);

    // the upload: [count jobs | output pointers]
    upload_.reset();
    upload_.add(num_jobs * sizeof(DevCountJob<Fr>));
    const size_t off_outs = upload_.add(count * sizeof(Fr*));
    unsigned char* meta = upload_.image();
    auto* h_jobs = reinterpret_cast<DevCountJob<Fr>*>(meta);
    auto* h_outs = reinterpret_cast<Fr**>(meta + off_outs);
    std::vector<const Fr*> tables(count);
    for (size_t l = 0, c = 0, j = 0; l < count; ++l) {
      for (size_t k = 0; k < lookups[l].num_inputs; ++k) h_jobs[j++] = {dev[c++], (uint32_t)l, 0};
      tables[l] = dev[c++];
      h_outs[l] = outs[l];
    }
    const unsigned char* d_meta = upload_image(upload_, meta_, stream_);

    PhaseClock clock(stream_);
    clock.begin(0);
    for (size_t l = 0; l < count; ++l)
      FrSort<Fr>::run(tables[l], (uint32_t)u, perm + l * u, sorted + l * u, work + off_sort, scratch, stream_);
    clock.end();
    clock.begin(1);
    TA_HIP(hipMemsetAsync(counters, 0, count * u * sizeof(uint32_t), stream_));
    TA_HIP(hipMemsetAsync(misses, 0, count * sizeof(unsigned long long), stream_));
    hipLaunchKernelGGL(ll_count_kernel<Fr>, dim3((unsigned)(num_jobs * bpj)), dim3(kLlBlock), 0, stream_,
                       reinterpret_cast<const DevCountJob<Fr>*>(d_meta), sorted, perm, (uint32_t)u, (uint32_t)bpj,
                       counters, misses);
    hipLaunchKernelGGL(ll_m_kernel<Fr>, dim3((unsigned)(count * bpm)), dim3(kLlBlock), 0, stream_,
                       reinterpret_cast<Fr* const*>(d_meta + off_outs), counters, (uint32_t)n, (uint32_t)u,
                       (uint32_t)bpm);
    clock.end();
    TA_HIP(hipGetLastError());
    copy_out(outs, out_m, count, n);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the miss counters");
    if (out_misses)
      TA_HIP(hipMemcpyAsync(out_misses, misses, count * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
    TA_HIP(hipStreamSynchronize(stream_));
    clock.sum(ms, 2);
  });
}

template <class Fr>
void LogLookup<Fr>::grand_sums(size_t n, size_t u, const Fr& beta, const Lookup* lookups, const Fr* const* m,
                               size_t count, const Fr* blinds, Fr* const* out_phi, Fr* out_totals, float* ms) {
  ms[2] = ms[3] = ms[4] = 0.f;
  if (!count) return;
  const size_t num_inputs = total_inputs<Fr>(lookups, count);
  const size_t tpj = ceil_div(n, kLlTile), tiles = count * tpj;
  drained_on_throw(stream_, [&] {
    if (tiles > kLlMaxBlocks) throw std::runtime_error("log lookup: too many tiles for one call");
    // device views: every lookup's inputs, its table, its m (u rows of each)
    std::vector<const Fr*> cols;
    for (size_t l = 0; l < count; ++l) {
      cols.insert(cols.end(), lookups[l].inputs, lookups[l].inputs + lookups[l].num_inputs);
      cols.push_back(lookups[l].table);
      cols.push_back(m[l]);
    }
    const std::vector<size_t> lens(cols.size(), u);
    const std::vector<const Fr*> dev = stage_columns(cols.data(), lens.data(), cols.size(), stage_, stream_);
    const std::vector<Fr*> outs = outputs(out_phi, count, n);

    // work_: per tile [sum of its terms | carry-in | 1 / product of denominators], every lookup's full sum, the blinds
    const size_t blind_bytes = count * (n - u - 1) * sizeof(Fr);
    Fr* sums = static_cast<Fr*>(work_.ensure((3 * tiles + count) * sizeof(Fr) + blind_bytes));
    Fr* carries = sums + tiles;
    Fr* dens = carries + tiles;
    Fr* totals = dens + tiles;
    Fr* d_blinds = totals + count;
    if (blind_bytes) TA_HIP(hipMemcpyAsync(d_blinds, blinds, blind_bytes, hipMemcpyDefault, stream_));

    // the upload: [jobs | input pointers]
    upload_.reset();
    upload_.add(count * sizeof(DevSumJob<Fr>));
    const size_t off_in = upload_.add(num_inputs * sizeof(Fr*));
    unsigned char* meta = upload_.image();
    auto* h_jobs = reinterpret_cast<DevSumJob<Fr>*>(meta);
    auto* h_in = reinterpret_cast<const Fr**>(meta + off_in);
    for (size_t l = 0, c = 0, f = 0; l < count; ++l) {
      h_jobs[l].begin = (uint32_t)f;
      for (size_t k = 0; k < lookups[l].num_inputs; ++k) h_in[f++] = dev[c++];
      h_jobs[l].end = (uint32_t)f;
      h_jobs[l].table = dev[c++];
      h_jobs[l].m = dev[c++];
      h_jobs[l].phi = outs[l];
    }
    const unsigned char* d_meta = upload_image(upload_, meta_, stream_);
    const auto* d_jobs = reinterpret_cast<const DevSumJob<Fr>*>(d_meta);

    PhaseClock clock(stream_);
    clock.begin(2);
    hipLaunchKernelGGL(ll_terms_kernel<Fr>, dim3((unsigned)tiles), dim3(kLlBlock), 0, stream_, d_jobs,
                       reinterpret_cast<const Fr* const*>(d_meta + off_in), beta, (uint32_t)u, (uint32_t)tpj, sums,
                       dens);
    hipLaunchKernelGGL(tile_invert_kernel<Fr>, dim3(ceil_div(tiles, 64)), dim3(64), 0, stream_, dens, sums,
                       (uint32_t)tiles);
    clock.end();
    clock.begin(3);
    hipLaunchKernelGGL(ll_carry_kernel<Fr>, dim3((unsigned)count), dim3(kLlBlock), 0, stream_, sums, carries, totals,
                       (uint32_t)tpj);
    clock.end();
    clock.begin(4);
    hipLaunchKernelGGL(ll_apply_kernel<Fr>, dim3((unsigned)tiles), dim3(kLlBlock), 0, stream_, d_jobs, carries, dens,
                       d_blinds, (uint32_t)n, (uint32_t)u, (uint32_t)tpj);
    clock.end();
    TA_HIP(hipGetLastError());
    copy_out(outs, out_phi, count, n);
    if (out_totals) TA_HIP(hipMemcpyAsync(out_totals, totals, count * sizeof(Fr), hipMemcpyDefault, stream_));
    TA_HIP(hipStreamSynchronize(stream_));
    clock.sum(ms, kLlPhases);
  });
}

template <class Fr>
size_t LogLookup<Fr>::work_bytes(size_t n, size_t max_inputs, size_t count) {
  if (!count || !n) return 0;
  const size_t column = n * sizeof(Fr), tiles = count * ceil_div(n, kLlTile);
  // m_polys: inputs and tables staged, m held, the sorted keys, permutations and counters, the sort's scratch
  const size_t m_call = count * (max_inputs + 1) * column + count * column +
                        align16(count * n * (sizeof(Fr) + 2 * sizeof(uint32_t)) + count * sizeof(uint64_t)) + 64 +
                        FrSort<Fr>::scratch(n, nullptr).total;
  // grand_sums: inputs, tables and m staged, phi held, the tile slots, the blinds
  const size_t sums_call = count * (max_inputs + 2) * column + count * column + (3 * tiles + count) * sizeof(Fr) +
                           count * column;
  return std::max(m_call, sums_call);
}

template class LogLookup<Bn254Fr>;
template class LogLookup<Bls381Fr>;

}  // namespace tachyon_amd::plonk
