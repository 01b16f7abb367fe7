// Grand-product polynomials: ratios, carry walk, apply (see grand_product.h
// for the definition and the three passes).
#include "grand_product.h"

#include <algorithm>
#include <cstring>

#include "../common/omega_table.h"
#include "../field/fr_device.h"
#include "tile_invert.h"

namespace tachyon_amd::plonk {

namespace {

constexpr unsigned kWaves = kGpBlock / 64;

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
#pragma unroll
    for (unsigned k = 0; k < kGpChunk; ++k) wrow[k] = omega_at<kGpBlock>(wtab, threadIdx.x, base / kGpBlock + k);
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
  const Fr before = block_scan_mul<Fr, kGpBlock, false>(run, lds, &total);
  Fr after = block_scan_mul<Fr, kGpBlock, true>(run, lds, &unused);  // then also this thread's den[k+1..]
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
  block_scan_mul<Fr, kGpBlock, false>(nprod, lds, &ntotal);
  if (threadIdx.x == 0) {
    store_fr(prods + blockIdx.x, ntotal);
    store_fr(dens + blockIdx.x, total);
  }
}

// Pass A, tiles: tile_invert_kernel (tile_invert.h), one lane per tile.
// dens[t] <- 1 / P_t, prods[t] <- the product of the tile's ratios.

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
    const Fr e = block_scan_mul<Fr, kGpBlock, false>(x, lds, &total);
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
  Fr acc = load_fr(carries + blockIdx.x) * block_scan_mul<Fr, kGpBlock, false>(p, lds, &total);
#pragma unroll
  for (unsigned k = 0; k < kGpChunk; ++k) {
    const uint32_t j = j0 + k;
    if (j <= u) store_fr(z + j, acc.canonical());
    else if (j < n) store_fr(z + j, load_fr(bl + (j - u - 1)));
    acc = acc * r[k];
  }
}

template <class Poly, class Fn>
void for_each_factor(const Poly& p, Fn&& fn) {
  for (size_t k = 0; k < p.num_count; ++k) fn(p.num[k]);
  for (size_t k = 0; k < p.den_count; ++k) fn(p.den[k]);
}

}  // namespace

// One run: its shape, the device views of its columns and outputs, its upload
template <class Fr>
struct GrandProduct<Fr>::Call {
  size_t n, u;
  const Poly* polys;
  const size_t* chain_lens;
  size_t num_chains;
  size_t num_polys = 0, num_factors = 0, tpj = 0, total_tiles = 0;
  bool any_label = false;
  std::vector<const Fr*> cols;  // per factor in the jobs' order: its values, then its table (kTable)
  std::vector<Fr*> z;           // per job: its rows on the device
  // the upload: [jobs | factors | chains | omega tables | blinds]
  size_t off_fac = 0, off_chain = 0, off_tab = 0, off_blind = 0;
  const unsigned char* d_meta = nullptr;
};

template <class Fr>
void GrandProduct<Fr>::run(size_t n, size_t u, const Fr& omega, const Fr& delta, const Poly* polys,
                           const size_t* chain_lens, size_t num_chains, const Fr* blinds, Fr* const* out_z,
                           Fr* out_last, float* ms) {
  float unread[3];
  if (!ms) ms = unread;
  ms[0] = ms[1] = ms[2] = 0.f;
  if (!num_chains) return;
  Call c{n, u, polys, chain_lens, num_chains};
  for (size_t i = 0; i < num_chains; ++i) c.num_polys += chain_lens[i];
  c.tpj = ceil_div(n, kGpTile);
  c.total_tiles = c.num_polys * c.tpj;
  drained_on_throw(stream_, [&] {
    if (c.total_tiles > kGpMaxTiles) throw std::runtime_error("grand product: too many tiles for one call");
    stage(c, out_z);
    pack(c, omega, delta, blinds);
    PhaseClock clock(stream_);
    launch(c, clock);
    copy_out(c, out_z, out_last);
    clock.sum(ms, 3);
  });
}

// Device views of the input columns, each distinct column once; the outputs
// in place where they are aligned device memory
template <class Fr>
void GrandProduct<Fr>::stage(Call& c, Fr* const* out_z) {
  std::vector<const Fr*> cols;
  for (size_t i = 0; i < c.num_polys; ++i)
    for_each_factor(c.polys[i], [&](const Factor& f) {
      cols.push_back(f.values);
      if (f.kind == kTable) cols.push_back(f.table);
      c.any_label |= f.kind == kLabel;
      ++c.num_factors;
    });
  const std::vector<size_t> lens(cols.size(), c.n);
  c.cols = stage_columns(cols.data(), lens.data(), cols.size(), stage_, stream_);
  size_t held = 0;
  for (size_t i = 0; i < c.num_polys; ++i) held += usable_in_place(out_z[i]) ? 0 : 1;
  Fr* res = held ? static_cast<Fr*>(result_.ensure(held * c.n * sizeof(Fr))) : nullptr;
  c.z.resize(c.num_polys);
  for (size_t i = 0, k = 0; i < c.num_polys; ++i) c.z[i] = usable_in_place(out_z[i]) ? out_z[i] : res + c.n * k++;
}

template <class Fr>
void GrandProduct<Fr>::pack(Call& c, const Fr& omega, const Fr& delta, const Fr* blinds) {
  const size_t blind_bytes = c.num_polys * (c.n - c.u - 1) * sizeof(Fr);
  upload_.reset();
  upload_.add(c.num_polys * sizeof(DevJob<Fr>));
  c.off_fac = upload_.add(c.num_factors * sizeof(DevFactor<Fr>));
  c.off_chain = upload_.add(c.num_chains * 2 * sizeof(uint32_t));
  c.off_tab = upload_.add(c.any_label ? omega_table_size(c.n, kGpBlock) * sizeof(Fr) : 0);
  c.off_blind = upload_.add(blind_bytes);
  unsigned char* meta = upload_.image();
  auto* h_jobs = reinterpret_cast<DevJob<Fr>*>(meta);
  auto* h_fac = reinterpret_cast<DevFactor<Fr>*>(meta + c.off_fac);
  auto* h_chain = reinterpret_cast<uint32_t*>(meta + c.off_chain);
  uint32_t nf = 0;
  const Fr* const* col = c.cols.data();
  for (size_t i = 0; i < c.num_polys; ++i) {
    DevJob<Fr>& job = h_jobs[i];
    job.begin = nf;
    job.num_end = nf + (uint32_t)c.polys[i].num_count;
    job.has_label = 0;
    job.z = c.z[i];
    for_each_factor(c.polys[i], [&](const Factor& f) {
      DevFactor<Fr>& o = h_fac[nf++];
      o.v = *col++;
      o.t = f.kind == kTable ? *col++ : nullptr;
      o.m = f.m;
      if (f.kind == kLabel) {
        o.m = (o.m * delta.pow(&f.label, 1)).canonical();
        job.has_label = 1;
      }
      o.c = f.c;
      o.kind = f.kind;
      o.pad = 0;
    });
    job.end = nf;
  }
  for (size_t i = 0, first = 0; i < c.num_chains; first += c.chain_lens[i++]) {
    h_chain[2 * i] = (uint32_t)(first * c.tpj);
    h_chain[2 * i + 1] = (uint32_t)(c.chain_lens[i] * c.tpj);
  }
  if (c.any_label) omega_table_fill(reinterpret_cast<Fr*>(meta + c.off_tab), c.n, kGpBlock, omega);
  if (blind_bytes) memcpy(meta + c.off_blind, blinds, blind_bytes);
  c.d_meta = upload_image(upload_, meta_, stream_);
}

// prods_: per tile [product of ratios | carry-in | 1 / product of denominators], then every chain's last value
template <class Fr>
void GrandProduct<Fr>::launch(const Call& c, PhaseClock& clock) {
  const size_t tiles = c.total_tiles;
  Fr* prods = static_cast<Fr*>(prods_.ensure((3 * tiles + c.num_chains) * sizeof(Fr)));
  Fr* carries = prods + tiles;
  Fr* dens = carries + tiles;
  const auto* d_jobs = reinterpret_cast<const DevJob<Fr>*>(c.d_meta);
  clock.begin(0);
  if (tiles) {
    hipLaunchKernelGGL(gp_ratio_kernel<Fr>, dim3((unsigned)tiles), dim3(kGpBlock), 0, stream_, d_jobs,
                       reinterpret_cast<const DevFactor<Fr>*>(c.d_meta + c.off_fac),
                       reinterpret_cast<const Fr*>(c.d_meta + c.off_tab), (uint32_t)c.u, (uint32_t)c.tpj, prods, dens);
    hipLaunchKernelGGL(tile_invert_kernel<Fr>, dim3(ceil_div(tiles, 64)), dim3(64), 0, stream_, dens, prods,
                       (uint32_t)tiles);
  }
  clock.end();
  clock.begin(1);
  hipLaunchKernelGGL(gp_carry_kernel<Fr>, dim3((unsigned)c.num_chains), dim3(kGpBlock), 0, stream_,
                     reinterpret_cast<const uint32_t*>(c.d_meta + c.off_chain), prods, carries, dens + tiles);
  clock.end();
  clock.begin(2);
  if (tiles)
    hipLaunchKernelGGL(gp_apply_kernel<Fr>, dim3((unsigned)tiles), dim3(kGpBlock), 0, stream_, d_jobs, carries, dens,
                       reinterpret_cast<const Fr*>(c.d_meta + c.off_blind), (uint32_t)c.n, (uint32_t)c.u,
                       (uint32_t)c.tpj);
  clock.end();
  TA_HIP(hipGetLastError());
}

template <class Fr>
void GrandProduct<Fr>::copy_out(const Call& c, Fr* const* out_z, Fr* out_last) {
  for (size_t i = 0; i < c.num_polys; ++i)
    if (c.z[i] != out_z[i]) TA_HIP(hipMemcpyAsync(out_z[i], c.z[i], c.n * sizeof(Fr), hipMemcpyDefault, stream_));
  if (out_last)
    TA_HIP(hipMemcpyAsync(out_last, prods_.template as<Fr>() + 3 * c.total_tiles, c.num_chains * sizeof(Fr),
                          hipMemcpyDeviceToHost, stream_));
  TA_HIP(hipStreamSynchronize(stream_));
}

template class GrandProduct<Bn254Fr>;
template class GrandProduct<Bls381Fr>;

}  // namespace tachyon_amd::plonk
