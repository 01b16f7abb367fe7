// Batched evaluation, linear combination and division by linear factors of
// dense polynomials over Fr (see poly_ops.h for the scheme and the tiling).
#include "poly_ops.h"

#include <algorithm>
#include <cstring>

#include "../field/fr_device.h"

namespace tachyon_amd::kzg {

namespace {

constexpr unsigned kWaves = kPolyBlock / 64;

// The thread's kPolyChunk coefficients from `base` (zero past len) and their
// Horner value h = sum_j a[j] z^j
template <class Fr>
__device__ __forceinline__ Fr load_chunk(const Fr* __restrict__ p, uint64_t len, uint64_t base, const Fr& z,
                                         Fr (&a)[kPolyChunk]) {
#pragma unroll
  for (unsigned j = 0; j < kPolyChunk; ++j) a[j] = base + j < len ? load_fr(p + base + j) : Fr::zero();
  Fr h = a[kPolyChunk - 1];
#pragma unroll
  for (int j = (int)kPolyChunk - 2; j >= 0; --j) h = a[j] + z * h;
  return h;
}

// Suffix scan over the workgroup's chunk values.  h: this thread's chunk
// value; carry: S at the tile's end (the same in every thread).  Returns
// S at the tile's start (in every thread) and sets *chunk_end to S at the end
// of this thread's chunk.  tab[k] = z^(kPolyChunk k), k = 1..64.
template <class Fr>
__device__ __forceinline__ Fr tile_suffix_scan(const Fr& h, const Fr* __restrict__ tab, const Fr& carry, Fr* lds,
                                               Fr* chunk_end) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // Kogge-Stone over the wave: s = sum_{i' >= lane} h_i' z^(chunk (i' - lane))
  Fr s = h;
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const Fr t = shfl_down_fr(s, d);
    const Fr m = s + load_fr(tab + d) * t;
    if (lane + d < 64) s = m;
  }
  __syncthreads();  // the previous tile's readers are done with lds
  if (lane == 0) lds[wave] = s;
  __syncthreads();
  // across the waves, from the top: acc = S at the end of wave w
  const Fr z64 = load_fr(tab + 64);
  Fr acc = carry, wave_end = carry;
#pragma unroll
  for (int w = (int)kWaves - 1; w >= 0; --w) {
    if ((unsigned)w == wave) wave_end = acc;
    acc = lds[w] + z64 * acc;
  }
  if (chunk_end) {
    // S at this thread's chunk start, then its neighbour's is this one's end
    const Fr full = s + load_fr(tab + (64 - lane)) * wave_end;
    const Fr next = shfl_down_fr(full, 1);
    *chunk_end = lane < 63 ? next : wave_end;
  }
  return acc;
}

template <class Fr>
struct EvalJob {
  const Fr* p;
  uint64_t len;
  const Fr* tab;
  Fr* out;  // one value per tile
};

// out[tile] = sum_{k in tile} p[k] z^(k - tile start); grid (tiles, jobs)
template <class Fr>
__global__ __launch_bounds__(kPolyBlock) void poly_eval_tiles_kernel(const EvalJob<Fr>* __restrict__ jobs) {
  __shared__ Fr lds[kWaves];
  const EvalJob<Fr> job = jobs[blockIdx.y];
  const uint64_t tile = blockIdx.x;
  if (tile * kPolyTile >= job.len && tile > 0) return;  // tile 0 of an empty polynomial writes 0
  Fr a[kPolyChunk];
  const Fr h = load_chunk(job.p, job.len, tile * kPolyTile + (uint64_t)threadIdx.x * kPolyChunk, load_fr(job.tab), a);
  const Fr total = tile_suffix_scan<Fr>(h, job.tab, Fr::zero(), lds, nullptr);
  if (threadIdx.x == 0) store_fr(job.out + tile, total.canonical());
}

// out[j - 1] = S_j for 1 <= j < len, *rem = S_0.  kSerial: one workgroup
// walks every tile from the top and carries S across them itself (the carry
// pass over the per-tile partials); else one workgroup per tile, the carry
// of tile t read from carries[t] (zero for the last tile).
template <class Fr, bool kSerial>
__global__ __launch_bounds__(kPolyBlock) void poly_divide_kernel(const Fr* __restrict__ p, uint64_t len,
                                                                 const Fr* __restrict__ tab,
                                                                 const Fr* __restrict__ carries, Fr* __restrict__ out,
                                                                 Fr* __restrict__ rem) {
  __shared__ Fr lds[kWaves];
  const uint64_t ntiles = (len + kPolyTile - 1) / kPolyTile;
  const Fr z = load_fr(tab);
  Fr carry = Fr::zero();
  uint64_t tile = kSerial ? ntiles - 1 : blockIdx.x;
  if (!kSerial && tile + 1 < ntiles) carry = load_fr(carries + tile);
  for (;;) {
    const uint64_t base = tile * kPolyTile + (uint64_t)threadIdx.x * kPolyChunk;
    Fr a[kPolyChunk], acc;
    const Fr h = load_chunk(p, len, base, z, a);
    carry = tile_suffix_scan<Fr>(h, tab, carry, lds, &acc);
#pragma unroll
    for (int j = (int)kPolyChunk - 1; j >= 0; --j) {
      acc = a[j] + z * acc;  // S at base + j
      const uint64_t idx = base + j;
      if (idx >= 1 && idx < len) store_fr(out + idx - 1, acc.canonical());
    }
    if (!kSerial || tile == 0) break;
    --tile;
  }
  if (rem && tile == 0 && threadIdx.x == 0) store_fr(rem, carry.canonical());
}

template <class Fr>
struct LcTerm {
  const Fr* p;
  uint64_t len;
  Fr c;
};

// out[k] = sum_i c_i P_i[k] - d [k == 0]; one thread per coefficient, the
// inputs taken four at a time so that their loads are in flight together
template <class Fr>
__global__ __launch_bounds__(kPolyBlock) void poly_lincomb_kernel(const LcTerm<Fr>* __restrict__ terms, uint32_t count,
                                                                  Fr d, Fr* __restrict__ out, uint64_t out_len) {
  const uint64_t k = (uint64_t)blockIdx.x * kPolyBlock + threadIdx.x;
  if (k >= out_len) return;
  Fr acc = Fr::zero();
  for (uint32_t i = 0; i < count; i += 4) {
    Fr x[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
      x[j] = i + j < count && k < terms[i + j].len ? load_fr(terms[i + j].p + k) : Fr::zero();
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
      if (i + j < count) acc = acc + terms[i + j].c * x[j];
  }
  if (k == 0) acc = acc - d;
  store_fr(out + k, acc.canonical());
}

}  // namespace

template <class Fr>
Fr PolyOps<Fr>::power_table(const Fr& z, Fr* tab) {
  tab[0] = z;
  Fr zc = z;
  for (unsigned s = 1; s < kPolyChunk; s <<= 1) zc = zc.sqr();
  tab[1] = zc.canonical();
  for (unsigned k = 2; k < kPolyTableSize; ++k) tab[k] = (tab[k - 1] * zc).canonical();
  Fr zt = tab[64];
  for (unsigned s = 1; s < kWaves; s <<= 1) zt = zt.sqr();
  return zt.canonical();
}

template <class Fr>
Fr* PolyOps<Fr>::upload(const void* host, size_t bytes, DeviceBuffer& buf) {
  pending_.emplace_back(static_cast<const unsigned char*>(host), static_cast<const unsigned char*>(host) + bytes);
  void* d = buf.ensure(bytes ? bytes : 1);
  if (bytes) TA_HIP(hipMemcpyAsync(d, pending_.back().data(), bytes, hipMemcpyHostToDevice, stream_));
  return static_cast<Fr*>(d);
}

template <class Fr>
void PolyOps<Fr>::synchronize() {
  TA_HIP(hipStreamSynchronize(stream_));
  pending_.clear();
}

template <class Fr>
void PolyOps<Fr>::stage(const Fr* const* ptrs, const size_t* lens, size_t count, std::vector<const Fr*>* dev) {
  *dev = stage_columns(ptrs, lens, count, stage_, stream_);
}

template <class Fr>
void PolyOps<Fr>::linear_combination(const Term* terms, size_t count, const Fr& d, Fr* out, size_t out_len) {
  if (!out_len) return;
  std::vector<LcTerm<Fr>> h(count);
  for (size_t i = 0; i < count; ++i) h[i] = {terms[i].p, terms[i].len, terms[i].c};
  const auto* d_terms = reinterpret_cast<const LcTerm<Fr>*>(upload(h.data(), count * sizeof(LcTerm<Fr>), lc_meta_));
  hipLaunchKernelGGL(poly_lincomb_kernel<Fr>, dim3(ceil_div(out_len, kPolyBlock)), dim3(kPolyBlock), 0, stream_,
                     d_terms, (uint32_t)count, d, out, (uint64_t)out_len);
  TA_HIP(hipGetLastError());
}

template <class Fr>
void PolyOps<Fr>::divide_by_roots(const Fr* a, size_t len, const Fr* roots, size_t nroots, Fr* out, Fr* d_rems) {
  if (d_rems && nroots) TA_HIP(hipMemsetAsync(d_rems, 0, nroots * sizeof(Fr), stream_));
  const size_t steps = std::min(len, nroots);  // a step on the empty polynomial leaves it empty, remainder 0
  if (!steps) return;
  // per root: the table of z for the tiles and of z^kPolyTile for the carry pass
  std::vector<Fr> tabs(steps * 2 * kPolyTableSize);
  for (size_t j = 0; j < steps; ++j) {
    const Fr zt = power_table(roots[j], &tabs[2 * j * kPolyTableSize]);
    power_table(zt, &tabs[(2 * j + 1) * kPolyTableSize]);
  }
  const Fr* d_tabs = upload(tabs.data(), tabs.size() * sizeof(Fr), div_meta_);
  const size_t max_tiles = ceil_div(len, kPolyTile);
  Fr* partials = static_cast<Fr*>(partials_.ensure(max_tiles * (sizeof(Fr) + sizeof(EvalJob<Fr>))));
  auto* d_job = reinterpret_cast<EvalJob<Fr>*>(partials + max_tiles);
  Fr* carries = static_cast<Fr*>(carries_.ensure(max_tiles * sizeof(Fr)));
  Fr* tmp[2] = {nullptr, nullptr};
  if (steps > 1)
    for (int i = 0; i < 2; ++i) tmp[i] = static_cast<Fr*>(tmp_[i].ensure(len * sizeof(Fr)));
  const Fr* src = a;
  size_t n = len;
  for (size_t j = 0; j < steps; ++j, --n) {
    // the last root's quotient goes to out; it is empty when nroots >= len
    Fr* dst = j + 1 == steps ? out : tmp[j & 1];
    const Fr* tab = d_tabs + 2 * j * kPolyTableSize;
    Fr* rem = d_rems ? d_rems + j : nullptr;
    const unsigned ntiles = ceil_div(n, kPolyTile);
    if (ntiles > 1) {
      // reduce: one partial per tile; carry: their quotient by (X - z^tile),
      // whose remainder is the polynomial's own
      const EvalJob<Fr> job{src, n, tab, partials};
      TA_HIP(hipMemcpyAsync(d_job, &pending_.emplace_back(reinterpret_cast<const unsigned char*>(&job),
                                                          reinterpret_cast<const unsigned char*>(&job + 1))[0],
                            sizeof(job), hipMemcpyHostToDevice, stream_));
      hipLaunchKernelGGL(poly_eval_tiles_kernel<Fr>, dim3(ntiles, 1), dim3(kPolyBlock), 0, stream_, d_job);
      hipLaunchKernelGGL((poly_divide_kernel<Fr, true>), dim3(1), dim3(kPolyBlock), 0, stream_, partials,
                         (uint64_t)ntiles, tab + kPolyTableSize, static_cast<const Fr*>(nullptr), carries, rem);
      rem = nullptr;
    }
    hipLaunchKernelGGL((poly_divide_kernel<Fr, false>), dim3(ntiles), dim3(kPolyBlock), 0, stream_, src, (uint64_t)n,
                       tab, carries, dst, rem);
    TA_HIP(hipGetLastError());
    src = dst;
  }
}

template <class Fr>
void PolyOps<Fr>::evaluate(const Pair* pairs, size_t m, Fr* host_out) {
  if (!m) return;
  constexpr size_t kMaxJobs = 32768;  // grid.y
  for (size_t start = 0; start < m; start += kMaxJobs) {
    const size_t cnt = std::min(kMaxJobs, m - start);
    std::vector<const Fr*> src(cnt);
    std::vector<uint64_t> lens(cnt);
    std::vector<Fr> mult(cnt);
    for (size_t i = 0; i < cnt; ++i) src[i] = pairs[start + i].p, lens[i] = pairs[start + i].len, mult[i] = pairs[start + i].z;
    const Fr* result = nullptr;
    for (int level = 0;; ++level) {
      size_t stride = 1;
      for (size_t i = 0; i < cnt; ++i) stride = std::max<size_t>(stride, ceil_div(lens[i], kPolyTile));
      // [tables | jobs] in one upload
      const size_t tab_bytes = cnt * kPolyTableSize * sizeof(Fr);
      std::vector<unsigned char> meta(tab_bytes + cnt * sizeof(EvalJob<Fr>));
      Fr* tabs = reinterpret_cast<Fr*>(meta.data());
      auto* jobs = reinterpret_cast<EvalJob<Fr>*>(meta.data() + tab_bytes);
      Fr* d_out = static_cast<Fr*>(ev_part_[level & 1].ensure(cnt * stride * sizeof(Fr)));
      unsigned char* d_meta = static_cast<unsigned char*>(ev_meta_.ensure(meta.size()));
      for (size_t i = 0; i < cnt; ++i) {
        mult[i] = power_table(mult[i], tabs + i * kPolyTableSize);
        jobs[i] = {src[i], lens[i], reinterpret_cast<const Fr*>(d_meta) + i * kPolyTableSize, d_out + i * stride};
        src[i] = d_out + i * stride;
        lens[i] = std::max<size_t>(1, ceil_div(lens[i], kPolyTile));
      }
      upload(meta.data(), meta.size(), ev_meta_);
      hipLaunchKernelGGL(poly_eval_tiles_kernel<Fr>, dim3((unsigned)stride, (unsigned)cnt), dim3(kPolyBlock), 0, stream_,
                         reinterpret_cast<const EvalJob<Fr>*>(d_meta + tab_bytes));
      TA_HIP(hipGetLastError());
      if (stride == 1) {
        result = d_out;
        break;
      }
    }
    TA_HIP(hipMemcpyAsync(host_out + start, result, cnt * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
    synchronize();
  }
}

template class PolyOps<Bn254Fr>;
template class PolyOps<Bls381Fr>;

}  // namespace tachyon_amd::kzg
