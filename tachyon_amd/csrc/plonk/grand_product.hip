// Grand-product polynomials: ratios, carry walk, apply (see grand_product.h
// for the definition and the three passes).
#include "grand_product.h"

#include <algorithm>
#include <cstring>
#include <unordered_map>

namespace tachyon_amd::plonk {

namespace {

constexpr unsigned kWaves = kGpBlock / 64;
// omega^j = A[j % kGpBlock] B[(j / kGpBlock) % kTabB] C[j / (kGpBlock kTabB)]
constexpr unsigned kTabB = 256;

// 32-byte elements move as two 16-byte accesses
template <class Fr>
__device__ __forceinline__ Fr load_fr(const Fr* p) {
  static_assert(sizeof(Fr) == 32, "grand_product: 8-limb scalar fields");
  const uint4 lo = reinterpret_cast<const uint4*>(p)[0];
  const uint4 hi = reinterpret_cast<const uint4*>(p)[1];
  Fr r;
  r.v[0] = lo.x, r.v[1] = lo.y, r.v[2] = lo.z, r.v[3] = lo.w;
  r.v[4] = hi.x, r.v[5] = hi.y, r.v[6] = hi.z, r.v[7] = hi.w;
  return r;
}

template <class Fr>
__device__ __forceinline__ void store_fr(Fr* p, const Fr& x) {
  reinterpret_cast<uint4*>(p)[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

template <class Fr>
__device__ __forceinline__ Fr shfl_fr(const Fr& x, unsigned src) {
  Fr r;
#pragma unroll
  for (int i = 0; i < Fr::N; ++i) r.v[i] = (uint32_t)__shfl((int)x.v[i], (int)(src & 63), 64);
  return r;
}

// Exclusive product scan over the workgroup in thread order (kReverse: from
// the last thread down): returns the product of x over the threads before
// this one, *total the product over all of them (the same in every thread).
// lds: kWaves elements; the leading barrier lets the previous use drain.
template <class Fr, bool kReverse>
__device__ __forceinline__ Fr block_scan_mul(const Fr& x, Fr* lds, Fr* total) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned pos = kReverse ? 63 - lane : lane;
  // Kogge-Stone over the wave: s = product over the positions <= pos
  Fr s = x;
  for (unsigned d = 1; d < 64; d <<= 1) {
    const Fr t = shfl_fr(s, kReverse ? lane + d : lane - d);
    const Fr m = s * t;
    if (pos >= d) s = m;
  }
  Fr e = shfl_fr(s, kReverse ? lane + 1 : lane - 1);
  if (pos == 0) e = Fr::one();
  __syncthreads();
  if (pos == 63) lds[wave] = s;
  __syncthreads();
  Fr before = Fr::one(), acc = Fr::one();
  for (unsigned i = 0; i < kWaves; ++i) {
    const unsigned w = kReverse ? kWaves - 1 - i : i;
    if (w == wave) before = acc;
    acc = acc * lds[w];
  }
  *total = acc;
  return before * e;
}

template <class Fr>
struct DevFactor {
  const Fr* v;
  const Fr* t;  // kTable
  Fr m;         // kLabel: m delta^label
  Fr c;
  uint32_t kind;
  uint32_t pad;
};

template <class Fr>
struct DevJob {
  uint32_t begin, num_end, end;  // factors [begin, num_end) numerator, [num_end, end) denominator
  uint32_t has_label;
  Fr* z;  // n rows, 16-byte aligned
};

// v + m t(j) + c for the factor's column value v at row j; w: omega^j
template <class Fr>
__device__ __forceinline__ Fr factor_value(const DevFactor<Fr>* fac, const Fr& v, uint32_t j, const Fr& w) {
  Fr x = v;
  if (fac->kind == 1) x = x + fac->m * load_fr(fac->t + j);
  else if (fac->kind == 2) x = x + fac->m * w;
  return x + fac->c;
}

// num[k], den[k]: the products of the job's factors at row base + k kGpBlock +
// thread (rows < u only).  The i-th numerator and the i-th denominator factor
// go together: where they are over the same column -- the permutation's v_i --
// it is loaded once for both.
template <class Fr>
__device__ __forceinline__ void multiply_factors(const DevFactor<Fr>* __restrict__ factors, const DevJob<Fr>& job,
                                                 uint32_t base, uint32_t u, const Fr (&wrow)[kGpChunk],
                                                 Fr (&num)[kGpChunk], Fr (&den)[kGpChunk]) {
  const uint32_t nnum = job.num_end - job.begin, nden = job.end - job.num_end;
  for (uint32_t f = 0; f < nnum || f < nden; ++f) {
    const DevFactor<Fr>* nf = f < nnum ? factors + job.begin + f : nullptr;
    const DevFactor<Fr>* df = f < nden ? factors + job.num_end + f : nullptr;
    const bool shared = nf && df && nf->v == df->v;
#pragma unroll
    for (unsigned k = 0; k < kGpChunk; ++k) {
      const uint32_t j = base + k * kGpBlock + threadIdx.x;
      if (j >= u) continue;
      Fr v = Fr::zero();
      if (nf) {
        v = load_fr(nf->v + j);
        num[k] = num[k] * factor_value(nf, v, j, wrow[k]);
      }
      if (df) {
        if (!shared) v = load_fr(df->v + j);
        den[k] = den[k] * factor_value(df, v, j, wrow[k]);
      }
    }
  }
}

// Pass A, rows.  grid: tiles_per_job x jobs, flat.  Thread t of tile T owns
// the rows T kGpTile + k kGpBlock + t (consecutive lanes read consecutive
// elements; nothing here depends on the order of a tile's rows).  Montgomery's
// trick across the tile without its inversion: with P the product of the
// tile's denominators (a zero one entering as 1) and E_r, S_r the products of
// those before and after row r, 1 / den_r = E_r S_r / P.  The row's
// q_r = num_r E_r S_r goes to the output's own row (0 where den_r = 0), P to
// dens[tile] and the product of the numerators (0 with a zero denominator
// among them) to prods[tile]: ratio_r = q_r / P, their product prods / P.
template <class Fr>
__global__ __launch_bounds__(kGpBlock) void gp_ratio_kernel(const DevJob<Fr>* __restrict__ jobs,
                                                            const DevFactor<Fr>* __restrict__ factors,
                                                            const Fr* __restrict__ wtab, uint32_t u,
                                                            uint32_t tiles_per_job, Fr* __restrict__ prods,
                                                            Fr* __restrict__ dens) {
  __shared__ Fr lds[kWaves];
  const uint32_t poly = blockIdx.x / tiles_per_job, tile = blockIdx.x - poly * tiles_per_job;
  const uint32_t base = tile * kGpTile;
  if (base >= u) {  // no row of the recurrence in this tile
    if (threadIdx.x == 0) {
      store_fr(prods + blockIdx.x, Fr::one());
      store_fr(dens + blockIdx.x, Fr::one());
    }
    return;
  }
  const DevJob<Fr> job = jobs[poly];
  Fr wrow[kGpChunk], num[kGpChunk], den[kGpChunk];
#pragma unroll
  for (unsigned k = 0; k < kGpChunk; ++k) wrow[k] = num[k] = den[k] = Fr::one();
  if (job.has_label) {
    const Fr wl = load_fr(wtab + threadIdx.x);
#pragma unroll
    for (unsigned k = 0; k < kGpChunk; ++k) {
      const uint32_t slab = base / kGpBlock + k;  // the same in the whole workgroup
      wrow[k] = wl * (load_fr(wtab + kGpBlock + slab % kTabB) * load_fr(wtab + kGpBlock + kTabB + slab / kTabB));
    }
  }
  multiply_factors<Fr>(factors, job, base, u, wrow, num, den);

  // a zero denominator enters the products as 1; pre[k]: this thread's den[0..k]
  uint32_t zeros = 0;
  Fr pre[kGpChunk], run = Fr::one();
#pragma unroll
  for (unsigned k = 0; k < kGpChunk; ++k) {
    if (den[k].is_zero()) {
      zeros |= 1u << k;
      den[k] = Fr::one();
    }
    run = run * den[k];
    pre[k] = run;
  }
  Fr total, unused;
  const Fr before = block_scan_mul<Fr, false>(run, lds, &total);
  Fr after = block_scan_mul<Fr, true>(run, lds, &unused);  // then also this thread's den[k+1..]
  Fr nprod = Fr::one();
#pragma unroll
  for (int k = (int)kGpChunk - 1; k >= 0; --k) {
    const bool zero = (zeros >> k) & 1;
    const Fr q = zero ? Fr::zero() : num[k] * ((k ? before * pre[k ? k - 1 : 0] : before) * after);
    after = after * den[k];
    nprod = nprod * (zero ? Fr::zero() : num[k]);  // rows >= u: 1
    const uint32_t j = base + k * kGpBlock + threadIdx.x;
    if (j < u) store_fr(job.z + j, q);
  }
  Fr ntotal;
  block_scan_mul<Fr, false>(nprod, lds, &ntotal);
  if (threadIdx.x == 0) {
    store_fr(prods + blockIdx.x, ntotal);
    store_fr(dens + blockIdx.x, total);
  }
}

// Pass A, tiles.  One lane per tile: the tile's one inversion, 64 of them per
// wave side by side (a Fermat inversion is a chain of ~380 dependent
// products: in the row kernel it held a whole workgroup's registers idle
// behind one lane).  dens[t] <- 1 / P_t, prods[t] <- the product of the tile's
// ratios.
template <class Fr>
__global__ __launch_bounds__(64) void gp_invert_kernel(Fr* __restrict__ dens, Fr* __restrict__ prods, uint32_t count) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  const Fr p = load_fr(dens + i);
  if (p.is_one()) return;  // a tile past the usable rows: 1 / 1, prods as it is
  const Fr inv = p.inverse();  // a product of nonzero values
  store_fr(dens + i, inv);
  store_fr(prods + i, load_fr(prods + i) * inv);
}

// Pass B.  One workgroup per chain: an exclusive product scan of the chain's
// tile products (its jobs' tiles are consecutive), kGpWalk at a time, the
// carry kept in registers from one step to the next.
template <class Fr>
__global__ __launch_bounds__(kGpBlock) void gp_carry_kernel(const uint32_t* __restrict__ chains,
                                                            const Fr* __restrict__ prods, Fr* __restrict__ carries,
                                                            Fr* __restrict__ last) {
  __shared__ Fr lds[kWaves];
  const uint32_t first = chains[2 * blockIdx.x], count = chains[2 * blockIdx.x + 1];
  Fr carry = Fr::one();
  for (uint32_t i0 = 0; i0 < count; i0 += kGpWalk) {
    const uint32_t i = i0 + threadIdx.x;
    const Fr x = i < count ? load_fr(prods + first + i) : Fr::one();
    Fr total;
    const Fr e = block_scan_mul<Fr, false>(x, lds, &total);
    if (i < count) store_fr(carries + first + i, carry * e);
    carry = carry * total;
  }
  if (threadIdx.x == 0) store_fr(last + blockIdx.x, carry.canonical());
}

// Pass C.  Thread t of tile T owns the rows T kGpTile + t kGpChunk + k: it
// reads its q_r (ratio_r = q_r invs[tile]), then writes z over the same rows.
template <class Fr>
__global__ __launch_bounds__(kGpBlock) void gp_apply_kernel(const DevJob<Fr>* __restrict__ jobs,
                                                            const Fr* __restrict__ carries,
                                                            const Fr* __restrict__ invs,
                                                            const Fr* __restrict__ blinds, uint32_t n, uint32_t u,
                                                            uint32_t tiles_per_job) {
  __shared__ Fr lds[kWaves];
  const uint32_t poly = blockIdx.x / tiles_per_job, tile = blockIdx.x - poly * tiles_per_job;
  const uint32_t base = tile * kGpTile, j0 = base + threadIdx.x * kGpChunk;
  Fr* z = jobs[poly].z;
  const Fr* bl = blinds + (size_t)poly * (n - u - 1);
  if (base > u) {  // blind rows only
#pragma unroll
    for (unsigned k = 0; k < kGpChunk; ++k)
      if (j0 + k < n) store_fr(z + j0 + k, load_fr(bl + (j0 + k - u - 1)));
    return;
  }
  const Fr inv = load_fr(invs + blockIdx.x);
  Fr r[kGpChunk], p = Fr::one();
#pragma unroll
  for (unsigned k = 0; k < kGpChunk; ++k) {
    r[k] = j0 + k < u ? load_fr(z + j0 + k) * inv : Fr::one();
    p = p * r[k];
  }
  Fr total;
  Fr acc = load_fr(carries + blockIdx.x) * block_scan_mul<Fr, false>(p, lds, &total);
#pragma unroll
  for (unsigned k = 0; k < kGpChunk; ++k) {
    const uint32_t j = j0 + k;
    if (j <= u) store_fr(z + j, acc.canonical());
    else if (j < n) store_fr(z + j, load_fr(bl + (j - u - 1)));
    acc = acc * r[k];
  }
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

template <class Fr>
void GrandProduct<Fr>::run(size_t n, size_t u, const Fr& omega, const Fr& delta, const Poly* polys,
                           const size_t* chain_lens, size_t num_chains, const Fr* blinds, Fr* const* out_z,
                           Fr* out_last, float* ms) {
  if (ms) ms[0] = ms[1] = ms[2] = 0.f;
  if (!num_chains) return;
  try {
    enqueue(n, u, omega, delta, polys, chain_lens, num_chains, blinds, out_z, out_last, ms);
  } catch (...) {
    (void)hipStreamSynchronize(stream_);  // nothing of the caller's stays in flight
    throw;
  }
}

template <class Fr>
void GrandProduct<Fr>::enqueue(size_t n, size_t u, const Fr& omega, const Fr& delta, const Poly* polys,
                               const size_t* chain_lens, size_t num_chains, const Fr* blinds, Fr* const* out_z,
                               Fr* out_last, float* ms) {
  size_t num_polys = 0;
  for (size_t c = 0; c < num_chains; ++c) num_polys += chain_lens[c];
  const size_t tpj = ceil_div(n, kGpTile), total_tiles = num_polys * tpj, nblind = n - u - 1;
  if (total_tiles > kGpMaxTiles) throw std::runtime_error("grand product: too many tiles for one call");

  // device views of the input columns: each distinct column once
  std::unordered_map<const Fr*, const Fr*> dev;
  auto note = [&](const Fr* p) {
    if (!dev.count(p)) dev[p] = usable(p) ? p : nullptr;
  };
  size_t num_factors = 0;
  bool any_label = false;
  for (size_t i = 0; i < num_polys; ++i) {
    for (int side = 0; side < 2; ++side) {
      const Factor* f = side ? polys[i].den : polys[i].num;
      const size_t cnt = side ? polys[i].den_count : polys[i].num_count;
      num_factors += cnt;
      for (size_t k = 0; k < cnt; ++k) {
        note(f[k].values);
        if (f[k].kind == kTable) note(f[k].table);
        any_label |= f[k].kind == kLabel;
      }
    }
  }
  size_t staged = 0;
  for (auto& kv : dev) staged += kv.second ? 0 : 1;
  if (staged) {
    Fr* d = static_cast<Fr*>(stage_.ensure(staged * n * sizeof(Fr)));
    for (auto& kv : dev) {
      if (kv.second) continue;
      TA_HIP(hipMemcpyAsync(d, kv.first, n * sizeof(Fr), hipMemcpyDefault, stream_));
      kv.second = d;
      d += n;
    }
  }
  // outputs: in place where they are aligned device memory
  std::vector<Fr*> z(num_polys);
  size_t held = 0;
  for (size_t i = 0; i < num_polys; ++i) held += usable(out_z[i]) ? 0 : 1;
  Fr* res = held ? static_cast<Fr*>(result_.ensure(held * n * sizeof(Fr))) : nullptr;
  for (size_t i = 0, k = 0; i < num_polys; ++i) z[i] = usable(out_z[i]) ? out_z[i] : res + n * k++;

  // one upload: [jobs | factors | chains | omega tables | blinds]
  const size_t tab_c = any_label ? ceil_div(n, (size_t)kGpBlock * kTabB) : 0;
  const size_t tab_len = any_label ? kGpBlock + kTabB + tab_c : 0;
  const size_t off_fac = align16(num_polys * sizeof(DevJob<Fr>));
  const size_t off_chain = align16(off_fac + num_factors * sizeof(DevFactor<Fr>));
  const size_t off_tab = align16(off_chain + num_chains * 2 * sizeof(uint32_t));
  const size_t off_blind = off_tab + tab_len * sizeof(Fr);
  const size_t meta_bytes = off_blind + num_polys * nblind * sizeof(Fr);
  std::vector<unsigned char>& meta = host_meta_;
  meta.assign(meta_bytes ? meta_bytes : 1, 0);
  unsigned char* d_meta = static_cast<unsigned char*>(meta_.ensure(meta.size()));
  auto* h_jobs = reinterpret_cast<DevJob<Fr>*>(meta.data());
  auto* h_fac = reinterpret_cast<DevFactor<Fr>*>(meta.data() + off_fac);
  auto* h_chain = reinterpret_cast<uint32_t*>(meta.data() + off_chain);
  Fr* h_tab = reinterpret_cast<Fr*>(meta.data() + off_tab);
  uint32_t nf = 0;
  for (size_t i = 0; i < num_polys; ++i) {
    DevJob<Fr>& job = h_jobs[i];
    job.begin = nf;
    job.has_label = 0;
    job.z = z[i];
    for (int side = 0; side < 2; ++side) {
      const Factor* f = side ? polys[i].den : polys[i].num;
      const size_t cnt = side ? polys[i].den_count : polys[i].num_count;
      for (size_t k = 0; k < cnt; ++k, ++nf) {
        DevFactor<Fr>& o = h_fac[nf];
        o.v = dev[f[k].values];
        o.t = f[k].kind == kTable ? dev[f[k].table] : nullptr;
        o.m = f[k].m;
        if (f[k].kind == kLabel) {
          o.m = (o.m * delta.pow(&f[k].label, 1)).canonical();
          job.has_label = 1;
        }
        o.c = f[k].c;
        o.kind = f[k].kind;
        o.pad = 0;
      }
      if (!side) job.num_end = nf;
    }
    job.end = nf;
  }
  for (size_t c = 0, first = 0; c < num_chains; first += chain_lens[c++]) {
    h_chain[2 * c] = (uint32_t)(first * tpj);
    h_chain[2 * c + 1] = (uint32_t)(chain_lens[c] * tpj);
  }
  if (any_label) {
    auto powers = [](Fr* out, size_t count, const Fr& step) {
      out[0] = Fr::one();
      for (size_t k = 1; k < count; ++k) out[k] = (out[k - 1] * step).canonical();
      return (out[count - 1] * step).canonical();
    };
    const Fr wb = powers(h_tab, kGpBlock, omega);
    const Fr wc = powers(h_tab + kGpBlock, kTabB, wb);
    powers(h_tab + kGpBlock + kTabB, tab_c, wc);
  }
  if (num_polys * nblind) memcpy(meta.data() + off_blind, blinds, num_polys * nblind * sizeof(Fr));
  TA_HIP(hipMemcpyAsync(d_meta, meta.data(), meta.size(), hipMemcpyHostToDevice, stream_));

  // per tile [product of ratios | carry-in | 1 / product of denominators], then every chain's last value
  Fr* prods = static_cast<Fr*>(prods_.ensure((3 * total_tiles + num_chains) * sizeof(Fr)));
  Fr* carries = prods + total_tiles;
  Fr* dens = carries + total_tiles;
  Fr* last = dens + total_tiles;
  const auto* d_jobs = reinterpret_cast<const DevJob<Fr>*>(d_meta);
  const auto* d_fac = reinterpret_cast<const DevFactor<Fr>*>(d_meta + off_fac);
  const auto* d_chain = reinterpret_cast<const uint32_t*>(d_meta + off_chain);
  const Fr* d_tab = reinterpret_cast<const Fr*>(d_meta + off_tab);
  const Fr* d_blind = reinterpret_cast<const Fr*>(d_meta + off_blind);

  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  auto mark = [&](int i) {
    if (!ms) return;
    TA_HIP(hipEventCreate(&ev[i]));
    TA_HIP(hipEventRecord(ev[i], stream_));
  };
  mark(0);
  if (total_tiles) {
    hipLaunchKernelGGL(gp_ratio_kernel<Fr>, dim3((unsigned)total_tiles), dim3(kGpBlock), 0, stream_, d_jobs, d_fac,
                       d_tab, (uint32_t)u, (uint32_t)tpj, prods, dens);
    hipLaunchKernelGGL(gp_invert_kernel<Fr>, dim3(ceil_div(total_tiles, 64)), dim3(64), 0, stream_, dens, prods,
                       (uint32_t)total_tiles);
  }
  mark(1);
  hipLaunchKernelGGL(gp_carry_kernel<Fr>, dim3((unsigned)num_chains), dim3(kGpBlock), 0, stream_, d_chain, prods,
                     carries, last);
  mark(2);
  if (total_tiles)
    hipLaunchKernelGGL(gp_apply_kernel<Fr>, dim3((unsigned)total_tiles), dim3(kGpBlock), 0, stream_, d_jobs, carries,
                       dens, d_blind, (uint32_t)n, (uint32_t)u, (uint32_t)tpj);
  mark(3);
  hipError_t err = hipGetLastError();
  for (size_t i = 0; i < num_polys && err == hipSuccess; ++i)
    if (z[i] != out_z[i]) err = hipMemcpyAsync(out_z[i], z[i], n * sizeof(Fr), hipMemcpyDefault, stream_);
  if (out_last && err == hipSuccess)
    err = hipMemcpyAsync(out_last, last, num_chains * sizeof(Fr), hipMemcpyDeviceToHost, stream_);
  if (err == hipSuccess) err = hipStreamSynchronize(stream_);
  if (ms && err == hipSuccess)
    for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  TA_HIP(err);
}

template class GrandProduct<Bn254Fr>;
template class GrandProduct<Bls381Fr>;

}  // namespace tachyon_amd::plonk
