// The Halo2 quotient: the program interpreter kernel, the scatter with the
// division, and the h(X) driver (see quotient.h).
#include "quotient.h"

#include <algorithm>
#include <cstring>
#include <unordered_map>

#include "../common/omega_table.h"
#include "../field/fr_device.h"
#include "../ntt/ntt.h"

namespace tachyon_amd::plonk {

namespace qp = quotient_plan;

namespace {

// What a lane needs besides the program: the read-only tables are separate
// __restrict__ kernel arguments, so that the compiler may fetch them by
// scalar loads while the kernel stores to acc and spill
template <class Fr>
struct EvalArgs {
  const Fr* consts;
  const Fr* const* cols;
  const Fr* spill;
  uint32_t n;
};

// One operand of the instruction in flight.  kind, index and rot are the
// same in every lane (they come from the instruction), so each case below is
// one branch for the wave; a constant is one address for the wave.
template <class Fr>
__device__ __forceinline__ Fr read_operand(const EvalArgs<Fr>& a, const uint4* lds, uint32_t kind, uint32_t index,
                                           uint32_t rot, uint32_t row, const Fr& acc, const Fr& xrow) {
  switch (kind) {
    case qp::kLConst: return a.consts[index];
    case qp::kLSlot:
      return unpack_fr<Fr>(lds[(index * 2) * kQBlock + threadIdx.x], lds[(index * 2 + 1) * kQBlock + threadIdx.x]);
    case qp::kLSpill: return load_fr(a.spill + (size_t)index * a.n + row);
    case qp::kLColumn: {
      uint32_t j = row + rot;  // rot < n <= 2^30
      if (j >= a.n) j -= a.n;
      // the pointer comes from a table, so the compiler would take it for a
      // generic one (flat loads wait on the LDS counter too); columns are
      // device memory, always
      typedef uint32_t U4 __attribute__((ext_vector_type(4)));
      using GlobalU4 = const __attribute__((address_space(1))) U4;
      GlobalU4* p = (GlobalU4*)(uintptr_t)(a.cols[index] + j);
      const U4 lo = p[0], hi = p[1];
      return unpack_fr<Fr>(lo, hi);
    }
    case qp::kLAcc: return acc;
    default: return xrow;
  }
}

// grid: ceil(n / kQBlock).  Lane t of block b owns row b kQBlock + t from the
// first instruction to the last: no lane reads another's slot, so there is no
// barrier.  Lanes past n (n < kQBlock only) compute on row 0 and store nothing.
template <class Fr>
__global__ __launch_bounds__(kQBlock) void quotient_eval_kernel(
    const qp::LInstr* __restrict__ code, const Fr* __restrict__ consts, const Fr* const* __restrict__ cols,
    const Fr* __restrict__ wtab, Fr* __restrict__ acc_rows, Fr* __restrict__ spill, uint32_t count, uint32_t n,
    uint32_t uses_xrow, const Fr xscale) {
  __shared__ uint4 lds[kQFastSlots * 2 * kQBlock];
  const EvalArgs<Fr> a{consts, cols, spill, n};
  const uint32_t at = blockIdx.x * kQBlock + threadIdx.x;
  const bool active = at < n;
  const uint32_t row = active ? at : 0;
  const Fr acc = load_fr(acc_rows + row);
  Fr xrow = Fr::zero();
  if (uses_xrow) {
    xrow = xscale * omega_at<kQBlock>(wtab, threadIdx.x, blockIdx.x);
  }
  Fr out = Fr::zero();
  auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); };  // the same in every lane
  for (uint32_t pc = 0; pc < count; ++pc) {
    const qp::LInstr ins = code[pc];
    const uint32_t op = uni(ins.op);
    const Fr x = read_operand(a, lds, uni(ins.a_kind), uni(ins.a), uni(ins.a_rot), row, acc, xrow);
    Fr r;
    if (op <= qp::kLMul) {
      const Fr y = read_operand(a, lds, uni(ins.b_kind), uni(ins.b), uni(ins.b_rot), row, acc, xrow);
      r = op == qp::kLAdd ? x + y : op == qp::kLSub ? x - y : x * y;
    } else if (op == qp::kLSquare) {
      r = x.sqr();
    } else if (op == qp::kLDouble) {
      r = x.dbl();
    } else if (op == qp::kLNegate) {
      r = -x;
    } else {
      r = x;
    }
    const uint32_t dst_kind = uni(ins.dst_kind), dst = uni(ins.dst);
    if (dst_kind == qp::kLSlot) {
      pack_fr(r, &lds[(dst * 2) * kQBlock + threadIdx.x], &lds[(dst * 2 + 1) * kQBlock + threadIdx.x]);
    } else if (dst_kind == qp::kLSpill) {
      if (active) store_fr(spill + (size_t)dst * n + row, r);
    } else {
      out = r;
    }
  }
  if (active) store_fr(acc_rows + row, out.canonical());
}

// The last kernel of a part: ext[j P + part] = acc[j] / (zeta^n w_ext^(n part) - 1)
template <class Fr>
__global__ __launch_bounds__(kQBlock) void quotient_scatter_kernel(const Fr* __restrict__ acc, Fr* __restrict__ ext,
                                                                   uint32_t n, uint32_t log_parts, uint32_t part,
                                                                   const Fr inv) {
  const uint32_t j = blockIdx.x * kQBlock + threadIdx.x;
  if (j >= n) return;
  store_fr(ext + (((size_t)j << log_parts) + part), (load_fr(acc + j) * inv).canonical());
}

// One term group, planned: its program, its constant table and the
// polynomials (or evaluations) behind its column table
template <class Fr>
struct GroupPlan {
  qp::Program prog;
  std::vector<Fr> consts;
  std::vector<const void*> cols;
  int phase = 1;
  size_t off_code = 0, off_consts = 0, off_cols = 0;  // in the upload
};

template <class Fr>
Fr from_bytes(const void* p) {
  Fr r;
  memcpy(&r, p, sizeof(Fr));
  return r;
}

// The field values the closed forms need, kept where their addresses stay
template <class Fr>
struct OwnConstants {
  Fr one = Fr::one(), zero = Fr::zero();
  std::vector<Fr> delta_pow;
  std::vector<const void*> delta_ptr;
  void set_delta(const Fr& delta, size_t m) {
    delta_pow.assign(m ? m : 1, Fr::one());
    for (size_t i = 1; i < m; ++i) delta_pow[i] = (delta_pow[i - 1] * delta).canonical();
    delta_ptr.clear();
    for (const Fr& d : delta_pow) delta_ptr.push_back(&d);
  }
};

// extras: l_first, l_last, l_active_row and the group's own columns
template <class Fr>
GroupPlan<Fr> plan_group(uint32_t kind, const qp::Params& p, const qp::Table& table, const qp::Graph* g1,
                         const qp::Graph* g2, const qp::Source* perm_cols, size_t m,
                         const std::vector<const void*>& extras, const OwnConstants<Fr>& own) {
  qp::Builder b;
  const qp::Source acc{qp::kAcc, 0, 0};
  qp::Source result;
  switch (kind) {
    case qp::kGates: {
      const qp::Source zero = b.constant(&own.zero);
      result = b.embed(*g1, acc, zero);
      break;
    }
    case qp::kPermutation:
      result = qp::build_permutation(b, acc, &own.one, perm_cols, m, p.cs_degree - 2, p.last_row, own.delta_ptr.data());
      break;
    case qp::kLookup: result = qp::build_lookup(b, acc, &own.one, &own.zero, *g1); break;
    default: result = qp::build_shuffle(b, acc, &own.one, &own.zero, *g1, *g2);
  }
  qp::Sizes sizes = qp::sizes_of(table);
  sizes.num_extra = extras.size();
  sizes.internal = true;
  GroupPlan<Fr> gp;
  gp.phase = 1 + (int)kind;
  gp.prog = qp::lower(b.view(), sizes, result, p.n, kQFastSlots);
  for (const void* c : b.constants) gp.consts.push_back(from_bytes<Fr>(c));
  for (size_t i = 0; i < table.num_challenges; ++i)
    gp.consts.push_back(from_bytes<Fr>(static_cast<const unsigned char*>(table.challenges) + i * sizeof(Fr)));
  for (const void* c : {p.beta, p.gamma, p.theta, p.y}) gp.consts.push_back(from_bytes<Fr>(c));
  for (size_t i = 0; i < table.num_fixed; ++i) gp.cols.push_back(table.fixed[i]);
  for (size_t i = 0; i < table.num_advice; ++i) gp.cols.push_back(table.advice[i]);
  for (size_t i = 0; i < table.num_instance; ++i) gp.cols.push_back(table.instance[i]);
  gp.cols.insert(gp.cols.end(), extras.begin(), extras.end());
  return gp;
}

// True for a group that changes the accumulator (a permutation over no column does not)
template <class Fr>
bool has_work(const GroupPlan<Fr>& g) {
  return !(g.prog.code.size() == 1 && g.prog.code[0].op == qp::kLCopy && g.prog.code[0].a_kind == qp::kLAcc);
}

// The groups of every circuit in the reference's order
template <class Fr>
std::vector<GroupPlan<Fr>> plan_call(const qp::Params& p, const qp::System& s, const qp::Circuit* circuits,
                                     size_t num_circuits, const OwnConstants<Fr>& own) {
  std::vector<GroupPlan<Fr>> groups;
  const std::vector<const void*> shared{p.l_first, p.l_last, p.l_active_row};
  auto add = [&](GroupPlan<Fr>&& g) {
    if (has_work(g)) groups.push_back(std::move(g));
  };
  for (size_t c = 0; c < num_circuits; ++c) {
    const qp::Circuit& ci = circuits[c];
    if (s.gates) add(plan_group<Fr>(qp::kGates, p, ci.table, s.gates, nullptr, nullptr, 0, {}, own));
    if (s.num_perm_columns) {
      std::vector<const void*> x = shared;
      x.insert(x.end(), ci.perm_z, ci.perm_z + ci.num_perm_z);
      x.insert(x.end(), s.sigmas, s.sigmas + s.num_perm_columns);
      add(plan_group<Fr>(qp::kPermutation, p, ci.table, nullptr, nullptr, s.perm_columns, s.num_perm_columns, x, own));
    }
    for (size_t k = 0; k < s.num_lookups; ++k) {
      std::vector<const void*> x = shared;
      x.insert(x.end(), {ci.lookup_z[k], ci.lookup_a_perm[k], ci.lookup_s_perm[k]});
      add(plan_group<Fr>(qp::kLookup, p, ci.table, &s.lookups[k], nullptr, nullptr, 0, x, own));
    }
    for (size_t k = 0; k < s.num_shuffles; ++k) {
      std::vector<const void*> x = shared;
      x.push_back(ci.shuffle_z[k]);
      add(plan_group<Fr>(qp::kShuffle, p, ci.table, &s.shuffles[2 * k], &s.shuffles[2 * k + 1], nullptr, 0, x, own));
    }
  }
  return groups;
}

// The upload of a call: every group's [code | constants | column pointers],
// then the omega power tables.  Fills the groups' offsets; returns the tables'.
template <class Fr>
size_t layout(SectionPacker& up, std::vector<GroupPlan<Fr>>& groups, size_t n) {
  up.reset();
  for (GroupPlan<Fr>& g : groups) {
    g.off_code = up.add(g.prog.code.size() * sizeof(qp::LInstr));
    g.off_consts = up.add(g.consts.size() * sizeof(Fr));
    g.off_cols = up.add(g.cols.size() * sizeof(void*));
  }
  return up.add(omega_table_size(n, kQBlock) * sizeof(Fr));
}

template <class Fr>
size_t spill_slots(const std::vector<GroupPlan<Fr>>& groups) {
  size_t s = 0;
  for (const GroupPlan<Fr>& g : groups) s = std::max(s, g.prog.spill_slots);
  return s;
}

// Each distinct polynomial of a call once, in the order of its first use
struct PolyList {
  std::vector<const void*> polys;
  std::unordered_map<const void*, size_t> index;
  size_t add(const void* p) {
    auto it = index.find(p);
    if (it != index.end()) return it->second;
    polys.push_back(p);
    return index[p] = polys.size() - 1;
  }
};

template <class Fr>
PolyList poly_list(const std::vector<GroupPlan<Fr>>& groups) {
  PolyList l;
  for (const GroupPlan<Fr>& g : groups)
    for (const void* c : g.cols) l.add(c);
  return l;
}

// Lays out, fills and enqueues the upload; device(col): the device address of
// a group's column.  Returns the device image; *off_tab: the tables' offset.
template <class Fr, class DeviceFn>
const unsigned char* upload_groups(SectionPacker& up, DeviceBuffer& buf, hipStream_t stream,
                                   std::vector<GroupPlan<Fr>>& groups, size_t n, const Fr& omega, size_t* off_tab,
                                   DeviceFn&& device) {
  *off_tab = layout(up, groups, n);
  unsigned char* meta = up.image();
  for (const GroupPlan<Fr>& g : groups) {
    memcpy(meta + g.off_code, g.prog.code.data(), g.prog.code.size() * sizeof(qp::LInstr));
    memcpy(meta + g.off_consts, g.consts.data(), g.consts.size() * sizeof(Fr));
    auto* cols = reinterpret_cast<const Fr**>(meta + g.off_cols);
    for (size_t i = 0; i < g.cols.size(); ++i) cols[i] = device(g.cols[i]);
  }
  omega_table_fill(reinterpret_cast<Fr*>(meta + *off_tab), n, kQBlock, omega);
  return upload_image(up, buf, stream);
}

template <class Fr>
void launch_group(const GroupPlan<Fr>& g, const unsigned char* d_meta, size_t off_tab, Fr* acc, Fr* spill, size_t n,
                  const Fr& xscale, hipStream_t stream) {
  hipLaunchKernelGGL(quotient_eval_kernel<Fr>, dim3(ceil_div(n, kQBlock)), dim3(kQBlock), 0, stream,
                     reinterpret_cast<const qp::LInstr*>(d_meta + g.off_code),
                     reinterpret_cast<const Fr*>(d_meta + g.off_consts),
                     reinterpret_cast<const Fr* const*>(d_meta + g.off_cols),
                     reinterpret_cast<const Fr*>(d_meta + off_tab), acc, spill, (uint32_t)g.prog.code.size(),
                     (uint32_t)n, (uint32_t)g.prog.uses_xrow, xscale);
}

// evaluate_part's one group
template <class Fr>
GroupPlan<Fr> plan_part(const qp::Params& params, const qp::Table& table, const qp::Group& group,
                        OwnConstants<Fr>& own) {
  const size_t m = group.num_perm_columns;
  if (group.kind == qp::kPermutation && m) own.set_delta(from_bytes<Fr>(group.delta), m);
  std::vector<const void*> extras;
  if (group.kind != qp::kGates) {
    extras = {params.l_first, params.l_last, params.l_active_row};
    extras.insert(extras.end(), group.z, group.z + group.num_z);
    if (group.kind == qp::kPermutation) extras.insert(extras.end(), group.sigmas, group.sigmas + m);
    if (group.kind == qp::kLookup) extras.insert(extras.end(), {group.a_perm, group.s_perm});
  }
  return plan_group<Fr>(group.kind, params, table, group.graph, group.graph2, group.perm_columns, m, extras, own);
}

}  // namespace

template <class Fr>
void Quotient<Fr>::program_stats(const qp::Params& params, const qp::Table& table, const qp::Group& group,
                                 size_t* out) {
  OwnConstants<Fr> own;
  const GroupPlan<Fr> g = plan_part<Fr>(params, table, group, own);
  out[0] = g.prog.code.size(), out[1] = g.prog.products, out[2] = g.prog.column_reads, out[3] = g.prog.slots_needed;
}

template <class Fr>
void Quotient<Fr>::evaluate_part(const qp::Params& params, const qp::Table& table, const qp::Group& group, void* acc,
                                 float* ms) {
  for (int i = 0; i < kQPhases; ++i) ms[i] = 0.f;
  const size_t n = params.n;
  OwnConstants<Fr> own;
  std::vector<GroupPlan<Fr>> groups;
  groups.push_back(plan_part<Fr>(params, table, group, own));
  if (!has_work(groups[0])) return;
  drained_on_throw(stream_, [&] {
    // what is not aligned device memory is staged: the columns each once, the accumulator apart from them
    PolyList list = poly_list(groups);
    const std::vector<size_t> lens(list.polys.size(), n);
    const auto dev = stage_columns(reinterpret_cast<const Fr* const*>(list.polys.data()), lens.data(), lens.size(),
                                   stage_, stream_);
    Fr* const host_acc = static_cast<Fr*>(acc);
    Fr* d_acc = stage_columns(&host_acc, &n, 1, acc_, stream_)[0];
    const Fr omega = group.omega ? from_bytes<Fr>(group.omega) : Fr::one();
    size_t off_tab = 0;
    const unsigned char* d_meta = upload_groups(upload_, meta_, stream_, groups, n, omega, &off_tab,
                                                [&](const void* p) { return dev[list.index[p]]; });
    const size_t spills = spill_slots(groups);
    Fr* spill = spills ? static_cast<Fr*>(spill_.ensure(spills * n * sizeof(Fr))) : nullptr;
    PhaseClock clock(stream_);
    clock.begin(groups[0].phase);
    launch_group(groups[0], d_meta, off_tab, d_acc, spill, n, group.x_scale ? from_bytes<Fr>(group.x_scale) : Fr::one(),
                 stream_);
    clock.end();
    TA_HIP(hipGetLastError());
    if (d_acc != acc) TA_HIP(hipMemcpyAsync(acc, d_acc, n * sizeof(Fr), hipMemcpyDefault, stream_));
    TA_HIP(hipStreamSynchronize(stream_));
    clock.sum(ms, kQPhases);
  });
}

template <class Fr>
size_t Quotient<Fr>::work_bytes(const qp::Params& params, const qp::System& system, const qp::Circuit* circuits,
                                size_t num_circuits) {
  OwnConstants<Fr> own;
  own.set_delta(Fr::one(), system.num_perm_columns);  // the plan's sizes do not depend on the values
  std::vector<GroupPlan<Fr>> groups = plan_call<Fr>(params, system, circuits, num_circuits, own);
  const size_t n = params.n, polys = poly_list(groups).polys.size();
  const uint32_t log_ext = qp::extended_log(n, params.cs_degree);
  const size_t N = size_t(1) << log_ext;
  SectionPacker up;
  layout(up, groups, n);
  const size_t meta = up.size();
  // cosets, the domain's scratch for the larger of the two transforms and its
  // tables (the domain's own bounds), ext, the accumulator, the spill rows
  using Dom = ntt::NttGenDomain<Fr>;
  const size_t scratch = std::max(Dom::scratch_bytes_bound(qp::log2_exact(n), polys), Dom::scratch_bytes_bound(log_ext, 1));
  return polys * n * sizeof(Fr) + scratch + N * sizeof(Fr) + n * sizeof(Fr) + spill_slots(groups) * n * sizeof(Fr) +
         meta + Dom::table_bytes_bound(log_ext) + 6 * 256;
}

template <class Fr>
void Quotient<Fr>::h_poly(const qp::Params& params, const qp::System& system, const qp::Circuit* circuits,
                          size_t num_circuits, const Fr& zeta, const Fr& delta, const Fr* ext_gen, bool full,
                          void* out, float* ms) {
  for (int i = 0; i < kQPhases; ++i) ms[i] = 0.f;
  const size_t n = params.n;
  const uint32_t log_n = qp::log2_exact(n), log_ext = qp::extended_log(n, params.cs_degree);
  const uint32_t log_parts = log_ext - log_n;
  const size_t parts = size_t(1) << log_parts, N = n << log_parts;
  OwnConstants<Fr> own;
  own.set_delta(delta, system.num_perm_columns);
  std::vector<GroupPlan<Fr>> groups = plan_call<Fr>(params, system, circuits, num_circuits, own);
  PolyList list = poly_list(groups);
  const size_t polys = list.polys.size();

  // one domain from the extended generator serves n and n P
  const Fr w_ext = ext_gen ? ext_gen->canonical() : ntt::root_of_unity<Fr>(log_ext);
  const uint64_t parts64 = parts;
  const uint32_t parts_limbs[2] = {(uint32_t)parts64, (uint32_t)(parts64 >> 32)};
  const Fr omega = w_ext.pow(parts_limbs, 2).canonical();
  // per part: 1 / (zeta^n w_ext^(n i) - 1); a zeta whose coset meets the
  // domain (X^n - 1 vanishes on a part) is refused before anything runs
  const uint64_t n64 = n;
  const uint32_t n_limbs[2] = {(uint32_t)n64, (uint32_t)(n64 >> 32)};
  const Fr w_ext_n = w_ext.pow(n_limbs, 2);
  std::vector<Fr> t_inv(parts);
  Fr cur_n = zeta.pow(n_limbs, 2).canonical();
  for (size_t i = 0; i < parts; ++i, cur_n = (cur_n * w_ext_n).canonical()) {
    if (cur_n.is_one()) throw std::runtime_error("quotient: zeta^n w_ext^(n i) = 1 on a part: X^n - 1 has no inverse there");
    t_inv[i] = (cur_n - Fr::one()).inverse().canonical();
  }
  ntt::NttGenDomain<Fr> dom(stream_);
  if (!dom.init(w_ext) || dom.log_order() != (int)log_ext)
    throw std::runtime_error("quotient: the extended generator's order is not 2^extended_k");

  drained_on_throw(stream_, [&] {
    Fr* cosets = static_cast<Fr*>(cosets_.ensure(std::max<size_t>(1, polys) * n * sizeof(Fr)));
    Fr* ext = static_cast<Fr*>(ext_.ensure(N * sizeof(Fr)));
    Fr* acc = static_cast<Fr*>(acc_.ensure(n * sizeof(Fr)));
    const size_t spills = spill_slots(groups);
    Fr* spill = spills ? static_cast<Fr*>(spill_.ensure(spills * n * sizeof(Fr))) : nullptr;
    size_t off_tab = 0;
    const unsigned char* d_meta = upload_groups(upload_, meta_, stream_, groups, n, omega, &off_tab,
                                                [&](const void* p) { return cosets + list.index[p] * n; });

    // per part: the coset zeta w_ext^i and the label scale delta_start w_ext^i
    const Fr beta = from_bytes<Fr>(params.beta);
    Fr cur = zeta.canonical();
    PhaseClock clock(stream_);
    constexpr size_t kMaxBatch = 65535;  // of one transform call
    for (size_t i = 0; i < parts; ++i) {
      clock.begin(0);
      for (size_t k = 0; k < polys; ++k)
        TA_HIP(hipMemcpyAsync(cosets + k * n, list.polys[k], n * sizeof(Fr), hipMemcpyDefault, stream_));
      for (size_t k = 0; k < polys; k += kMaxBatch)
        dom.run(cosets + k * n, log_n, false, std::min(kMaxBatch, polys - k), cur);
      clock.end();
      TA_HIP(hipMemsetAsync(acc, 0, n * sizeof(Fr), stream_));
      const Fr xscale = (beta * cur).canonical();
      for (const GroupPlan<Fr>& g : groups) {
        clock.begin(g.phase);
        launch_group(g, d_meta, off_tab, acc, spill, n, xscale, stream_);
        clock.end();
      }
      clock.begin(5);
      hipLaunchKernelGGL(quotient_scatter_kernel<Fr>, dim3(ceil_div(n, kQBlock)), dim3(kQBlock), 0, stream_, acc, ext,
                         (uint32_t)n, log_parts, (uint32_t)i, t_inv[i]);
      clock.end();
      TA_HIP(hipGetLastError());
      cur = (cur * w_ext).canonical();
    }
    clock.begin(6);
    dom.run(ext, log_ext, true, 1, zeta.canonical());
    clock.end();
    const size_t count = full ? N : n * (size_t)(params.cs_degree - 1);
    TA_HIP(hipMemcpyAsync(out, ext, count * sizeof(Fr), hipMemcpyDefault, stream_));
    TA_HIP(hipStreamSynchronize(stream_));
    clock.sum(ms, kQPhases);
    held_ = cosets_.capacity() + ext_.capacity() + acc_.capacity() + spill_.capacity() + meta_.capacity() +
            stage_.capacity() + dom.table_bytes() + dom.scratch_bytes();
  });
}

template class Quotient<Bn254Fr>;
template class Quotient<Bls381Fr>;

}  // namespace tachyon_amd::plonk
