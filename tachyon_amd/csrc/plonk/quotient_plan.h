// Host planner of the Halo2 quotient (include/tachyon_mi355x.h, "PLONK
// quotient"): host-only C++17 with no HIP dependency, so the
// refusal rules, the lowering and its interpreter compile and run on their own
// (check/quotient_plan_check.cc).
//
// Reference: zk/plonk/vanishing/graph_evaluator.h:60-76 (a graph's value on a
// row), calculation.h:71-104 (the ops), value_source.h (the operand kinds),
// permutation_evaluator.h:25-108, lookup/halo2/evaluator.h:66-128,
// shuffle/evaluator.h:71-119 (the closed forms) and circuit_polynomial_builder
// .h:199-245 (their order).
//
// Three parts:
//   validation  graph_ok / part_ok / h_poly_ok: everything the C-ABI refuses,
//               decided before any GPU call; only descriptor arrays are read.
//   Builder     one term group as ONE graph: the caller's graphs embedded, the
//               closed forms written as calculations over three internal
//               operand kinds (an extra column, the accumulator, the
//               permutation's row label).
//   lower       a graph to a flat program: Store becomes an alias, Horner a
//               Mul / Add chain in place, uniform values (constants,
//               challenges, beta, gamma, theta, y) one constant table, and
//               every computed value a slot, allocated lowest-free at its
//               definition and freed at its last use, so slots_needed is the
//               largest number of values live at once.  run_row interprets
//               a program on one row over any field type.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/tachyon_mi355x.h"

namespace tachyon_amd::quotient_plan {

using Source = tachyon_mi355x_quotient_source;
using Calc = tachyon_mi355x_quotient_calc;
using Graph = tachyon_mi355x_quotient_graph;
using Table = tachyon_mi355x_quotient_table;
using Params = tachyon_mi355x_quotient_params;
using Group = tachyon_mi355x_quotient_group;
using System = tachyon_mi355x_quotient_system;
using Circuit = tachyon_mi355x_quotient_circuit;

enum Kind : uint32_t {
  kConstant = 0,
  kIntermediate = 1,
  kFixed = 2,
  kAdvice = 3,
  kInstance = 4,
  kChallenge = 5,
  kBeta = 6,
  kGamma = 7,
  kTheta = 8,
  kY = 9,
  kPreviousValue = 10,
  kPublicKinds = 11,
  // the Builder's own: a column of the group's extra list, the label
  // x_scale omega^row, the accumulator
  kExtra = 11,
  kXRow = 12,
  kAcc = 13,
  kAllKinds = 14,
};
enum Op : uint32_t { kAdd = 0, kSub, kMul, kSquare, kDouble, kNegate, kHorner, kStore, kNumOps };
enum GroupKind : uint32_t { kGates = 0, kPermutation, kLookup, kShuffle, kNumGroups };

inline constexpr size_t kMaxLogN = 30;

struct Sizes {
  size_t num_fixed = 0, num_advice = 0, num_instance = 0, num_challenges = 0, num_extra = 0;
  bool internal = false;  // the Builder's kinds allowed
};

inline Sizes sizes_of(const Table& t) {
  return {t.num_fixed, t.num_advice, t.num_instance, t.num_challenges, 0, false};
}

inline bool is_column(uint32_t kind) {
  return kind == kFixed || kind == kAdvice || kind == kInstance || kind == kExtra;
}

inline bool source_ok(const Source& s, const Graph& g, const Sizes& t, const std::vector<char>& written) {
  if (s.kind >= (t.internal ? (uint32_t)kAllKinds : (uint32_t)kPublicKinds)) return false;
  switch (s.kind) {
    case kConstant: return s.index < g.num_constants;
    case kIntermediate: return s.index < g.num_intermediates && written[s.index];
    case kFixed: return s.index < t.num_fixed && s.rotation_index < g.num_rotations;
    case kAdvice: return s.index < t.num_advice && s.rotation_index < g.num_rotations;
    case kInstance: return s.index < t.num_instance && s.rotation_index < g.num_rotations;
    case kExtra: return s.index < t.num_extra && s.rotation_index < g.num_rotations;
    case kChallenge: return s.index < t.num_challenges;
    default: return true;
  }
}

// True for a graph every calculation of which can run in order
inline bool graph_ok(const Graph& g, const Sizes& t) {
  if ((g.num_calcs && !g.calcs) || (g.num_parts && !g.parts) || (g.num_constants && !g.constants) ||
      (g.num_rotations && !g.rotations))
    return false;
  if (g.num_calcs > UINT32_MAX || g.num_parts > UINT32_MAX || g.num_constants > UINT32_MAX ||
      g.num_rotations > UINT32_MAX || g.num_intermediates > UINT32_MAX)
    return false;
  std::vector<char> written(g.num_intermediates, 0);
  for (size_t i = 0; i < g.num_calcs; ++i) {
    const Calc& c = g.calcs[i];
    if (c.op >= kNumOps || c.target >= g.num_intermediates) return false;
    if (!source_ok(c.a, g, t, written)) return false;
    if (c.op == kAdd || c.op == kSub || c.op == kMul || c.op == kHorner)
      if (!source_ok(c.b, g, t, written)) return false;
    if (c.op == kHorner) {
      if (c.parts_begin > g.num_parts || c.parts_count > g.num_parts - c.parts_begin) return false;
      for (uint32_t k = 0; k < c.parts_count; ++k)
        if (!source_ok(g.parts[c.parts_begin + k], g, t, written)) return false;
    }
    written[c.target] = 1;
  }
  return true;
}

inline bool table_ok(const Table& t) {
  return !((t.num_fixed && !t.fixed) || (t.num_advice && !t.advice) || (t.num_instance && !t.instance) ||
           (t.num_challenges && !t.challenges));
}

inline bool columns_ok(const void* const* cols, size_t count) {
  if (count && !cols) return false;
  for (size_t i = 0; i < count; ++i)
    if (!cols[i]) return false;
  return true;
}

inline bool table_columns_ok(const Table& t) {
  return table_ok(t) && columns_ok(t.fixed, t.num_fixed) && columns_ok(t.advice, t.num_advice) &&
         columns_ok(t.instance, t.num_instance);
}

inline uint32_t log2_exact(size_t n) {
  uint32_t l = 0;
  while ((size_t(1) << l) < n) ++l;
  return l;
}

// the least e with 2^e >= n (cs_degree - 1) (halo2's extended_k)
inline uint32_t extended_log(size_t n, uint32_t cs_degree) {
  uint32_t e = log2_exact(n);
  while (e < 63 && (size_t(1) << e) < n * (size_t)(cs_degree - 1)) ++e;
  return e;
}

// field, n, cs_degree and the shared pointers; two_adicity: of the field
inline bool params_ok(const Params* p, bool need_domain, uint32_t two_adicity) {
  if (!p) return false;
  if (p->field != 0 && p->field != 2) return false;
  if (p->n < 2 || (p->n & (p->n - 1)) != 0 || p->n > (size_t(1) << kMaxLogN)) return false;
  if (p->cs_degree < 3) return false;
  if (need_domain) {
    const uint32_t e = extended_log(p->n, p->cs_degree);
    if (e > two_adicity || e > kMaxLogN) return false;
  }
  return p->theta && p->beta && p->gamma && p->y;
}

inline size_t perm_z_count(size_t m, uint32_t cs_degree) {
  const size_t L = cs_degree - 2;
  return (m + L - 1) / L;
}

inline bool perm_columns_ok(const Source* cols, size_t m, const void* const* sigmas, const Table& t) {
  if (m == 0) return true;
  if (!cols || !columns_ok(sigmas, m)) return false;
  for (size_t i = 0; i < m; ++i) {
    const size_t cnt = cols[i].kind == kFixed     ? t.num_fixed
                       : cols[i].kind == kAdvice  ? t.num_advice
                       : cols[i].kind == kInstance ? t.num_instance
                                                  : 0;  // another kind names no column
    if (cols[i].index >= cnt) return false;
  }
  return true;
}

// tachyon_mi355x_quotient_evaluate_part
inline bool part_ok(const Params* p, const Table* table, const Group* g, const void* acc, uint32_t two_adicity) {
  if (!params_ok(p, false, two_adicity) || !table || !g || !acc) return false;
  if (!table_columns_ok(*table) || g->kind >= kNumGroups) return false;
  const Sizes t = sizes_of(*table);
  const bool closed = g->kind != kGates;
  if (closed && (!p->l_first || !p->l_last || !p->l_active_row)) return false;
  switch (g->kind) {
    case kGates: return g->graph && graph_ok(*g->graph, t);
    case kPermutation:
      if (!perm_columns_ok(g->perm_columns, g->num_perm_columns, g->sigmas, *table)) return false;
      if (g->num_z != perm_z_count(g->num_perm_columns, p->cs_degree)) return false;
      if (g->num_perm_columns && (!g->x_scale || !g->omega || !g->delta)) return false;
      return columns_ok(g->z, g->num_z);
    case kLookup:
      return g->graph && graph_ok(*g->graph, t) && g->num_z == 1 && columns_ok(g->z, 1) && g->a_perm && g->s_perm;
    default:
      return g->graph && g->graph2 && graph_ok(*g->graph, t) && graph_ok(*g->graph2, t) && g->num_z == 1 &&
             columns_ok(g->z, 1);
  }
}

// tachyon_mi355x_quotient_h_poly
inline bool h_poly_ok(const Params* p, const System* s, const Circuit* circuits, size_t num_circuits, const void* zeta,
                      const void* delta, const void* out, uint32_t two_adicity) {
  if (!params_ok(p, true, two_adicity) || !s || !zeta || !out) return false;
  if (!p->l_first || !p->l_last || !p->l_active_row) return false;
  if (num_circuits && !circuits) return false;
  if ((s->num_lookups && !s->lookups) || (s->num_shuffles && !s->shuffles)) return false;
  if (s->num_perm_columns && !delta) return false;
  for (size_t c = 0; c < num_circuits; ++c) {
    const Circuit& ci = circuits[c];
    if (!table_columns_ok(ci.table)) return false;
    const Sizes t = sizes_of(ci.table);
    if (s->gates && !graph_ok(*s->gates, t)) return false;
    if (!perm_columns_ok(s->perm_columns, s->num_perm_columns, s->sigmas, ci.table)) return false;
    if (ci.num_perm_z != perm_z_count(s->num_perm_columns, p->cs_degree)) return false;
    if (!columns_ok(ci.perm_z, ci.num_perm_z)) return false;
    for (size_t k = 0; k < s->num_lookups; ++k)
      if (!graph_ok(s->lookups[k], t)) return false;
    if (!columns_ok(ci.lookup_z, s->num_lookups) || !columns_ok(ci.lookup_a_perm, s->num_lookups) ||
        !columns_ok(ci.lookup_s_perm, s->num_lookups))
      return false;
    for (size_t k = 0; k < 2 * s->num_shuffles; ++k)
      if (!graph_ok(s->shuffles[k], t)) return false;
    if (!columns_ok(ci.shuffle_z, s->num_shuffles)) return false;
  }
  return true;
}

// ---------------------------------------------------------------------------
// Builder: one term group as one graph.  Constants are kept as pointers to
// their 32-byte values (a caller's graph constants in place, the driver's own
// in its storage), so nothing here knows the field.

struct Builder {
  std::vector<Calc> calcs;
  std::vector<Source> parts;
  std::vector<const void*> constants;
  std::vector<int32_t> rotations;
  uint32_t num_intermediates = 0;
  size_t elem_bytes = 32;

  // For graph_ok and lower, which read a graph's constant COUNT only: the
  // `constants` field points at the pointer list, not at element values.
  Graph view() const {
    const void* list = constants.empty() ? nullptr : (const void*)constants.data();
    return {calcs.data(),     calcs.size(),     parts.data(),     parts.size(), list, constants.size(),
            rotations.data(), rotations.size(), num_intermediates};
  }
  uint32_t rotation(int32_t r) {
    for (size_t i = 0; i < rotations.size(); ++i)
      if (rotations[i] == r) return (uint32_t)i;
    rotations.push_back(r);
    return (uint32_t)rotations.size() - 1;
  }
  Source constant(const void* value) {
    constants.push_back(value);
    return {kConstant, (uint32_t)constants.size() - 1, 0};
  }
  Source extra(uint32_t index, int32_t rot = 0) { return {kExtra, index, rotation(rot)}; }
  Source emit(uint32_t op, Source a, Source b = Source{0, 0, 0}) {
    const uint32_t target = num_intermediates++;
    calcs.push_back({op, a, b, 0, 0, target});
    return {kIntermediate, target, 0};
  }
  // acc y + term
  Source fold(Source acc, Source term) { return emit(kAdd, emit(kMul, acc, Source{kY, 0, 0}), term); }

  // Appends g (validated) with its constants, rotations and intermediates
  // renumbered and PreviousValue replaced by `prev`.  Returns g's value:
  // its last target, or `zero` for a graph with no calculation.
  Source embed(const Graph& g, Source prev, Source zero) {
    const uint32_t c0 = (uint32_t)constants.size(), i0 = num_intermediates, p0 = (uint32_t)parts.size();
    for (size_t i = 0; i < g.num_constants; ++i)
      constants.push_back(static_cast<const unsigned char*>(g.constants) + i * elem_bytes);
    std::vector<uint32_t> rot(g.num_rotations);
    for (size_t i = 0; i < g.num_rotations; ++i) rot[i] = rotation(g.rotations[i]);
    auto map = [&](Source s) {
      if (s.kind == kConstant) s.index += c0;
      else if (s.kind == kIntermediate) s.index += i0;
      else if (s.kind == kPreviousValue) return prev;
      else if (is_column(s.kind)) s.rotation_index = rot[s.rotation_index];
      return s;
    };
    for (size_t i = 0; i < g.num_parts; ++i) parts.push_back(map(g.parts[i]));
    for (size_t i = 0; i < g.num_calcs; ++i) {
      Calc c = g.calcs[i];
      c.a = map(c.a);
      if (c.op == kAdd || c.op == kSub || c.op == kMul || c.op == kHorner) c.b = map(c.b);
      else c.b = Source{0, 0, 0};
      c.parts_begin = c.op == kHorner ? c.parts_begin + p0 : 0;
      if (c.op != kHorner) c.parts_count = 0;
      c.target += i0;
      calcs.push_back(c);
    }
    num_intermediates += (uint32_t)g.num_intermediates;
    return g.num_calcs ? Source{kIntermediate, g.calcs[g.num_calcs - 1].target + i0, 0} : zero;
  }
};

// The extra columns of a closed form: l_first, l_last, l_active_row, then
//   permutation  z_0 .. z_(k-1), sigma_0 .. sigma_(m-1)
//   lookup       z, a', s'
//   shuffle      z
enum : uint32_t { kXFirst = 0, kXLast = 1, kXActive = 2, kXGroup = 3 };

// l_first (1 - z), then l_last (z^2 - z) for zl (lookup, shuffle: the same z)
inline Source fold_boundaries(Builder& b, Source acc, Source one, Source z, Source zl) {
  acc = b.fold(acc, b.emit(kMul, b.emit(kSub, one, z), b.extra(kXFirst)));
  return b.fold(acc, b.emit(kMul, b.extra(kXLast), b.emit(kSub, b.emit(kSquare, zl), zl)));
}

// permutation_evaluator.h:25-108.  cols: the m permutation columns (table
// kinds); delta_pow[k]: the value delta^k (k >= 1 used); L = cs_degree - 2.
inline Source build_permutation(Builder& b, Source acc, const void* one, const Source* cols, size_t m, size_t L,
                                int32_t last_row, const void* const* delta_pow) {
  if (m == 0) return acc;
  const size_t k = (m + L - 1) / L;
  const Source c_one = b.constant(one);
  auto z = [&](size_t j, int32_t rot = 0) { return b.extra(kXGroup + (uint32_t)j, rot); };
  acc = fold_boundaries(b, acc, c_one, z(0), z(k - 1));
  for (size_t j = 1; j < k; ++j)
    acc = b.fold(acc, b.emit(kMul, b.extra(kXFirst), b.emit(kSub, z(j), z(j - 1, last_row))));
  const Source beta{kBeta, 0, 0}, gamma{kGamma, 0, 0}, xrow{kXRow, 0, 0};
  for (size_t j = 0; j < k; ++j) {
    const size_t lo = j * L, hi = std::min(m, lo + L);
    Source left = z(j, 1);
    for (size_t i = lo; i < hi; ++i) {
      Source col = cols[i];
      col.rotation_index = b.rotation(0);
      const Source sigma = b.extra(kXGroup + (uint32_t)(k + i));
      left = b.emit(kMul, left, b.emit(kAdd, b.emit(kAdd, col, b.emit(kMul, beta, sigma)), gamma));
    }
    Source right = z(j);
    for (size_t i = lo; i < hi; ++i) {
      Source col = cols[i];
      col.rotation_index = b.rotation(0);
      const Source label = i == 0 ? xrow : b.emit(kMul, xrow, b.constant(delta_pow[i]));
      right = b.emit(kMul, right, b.emit(kAdd, b.emit(kAdd, col, label), gamma));
    }
    acc = b.fold(acc, b.emit(kMul, b.emit(kSub, left, right), b.extra(kXActive)));
  }
  return acc;
}

// lookup/halo2/evaluator.h:66-128 over the argument's graph (its value: the
// compressed (A + beta)(S + gamma))
inline Source build_lookup(Builder& b, Source acc, const void* one, const void* zero, const Graph& g) {
  const Source c_one = b.constant(one), c_zero = b.constant(zero);
  const Source table_value = b.embed(g, c_zero, c_zero);
  const Source z = b.extra(kXGroup), a = b.extra(kXGroup + 1), s = b.extra(kXGroup + 2);
  acc = fold_boundaries(b, acc, c_one, z, z);
  const Source left = b.emit(kMul, b.emit(kMul, b.extra(kXGroup, 1), b.emit(kAdd, a, Source{kBeta, 0, 0})),
                             b.emit(kAdd, s, Source{kGamma, 0, 0}));
  acc = b.fold(acc, b.emit(kMul, b.extra(kXActive), b.emit(kSub, left, b.emit(kMul, z, table_value))));
  const Source a_minus_s = b.emit(kSub, a, s);
  acc = b.fold(acc, b.emit(kMul, b.extra(kXFirst), a_minus_s));
  const Source a_step = b.emit(kSub, a, b.extra(kXGroup + 1, -1));
  return b.fold(acc, b.emit(kMul, b.emit(kMul, b.extra(kXActive), a_minus_s), a_step));
}

// shuffle/evaluator.h:71-119 over the input's and the shuffle's graphs
inline Source build_shuffle(Builder& b, Source acc, const void* one, const void* zero, const Graph& g_input,
                            const Graph& g_shuffle) {
  const Source c_one = b.constant(one), c_zero = b.constant(zero);
  const Source input_value = b.embed(g_input, c_zero, c_zero);
  const Source value = b.embed(g_shuffle, c_zero, c_zero);
  const Source z = b.extra(kXGroup);
  acc = fold_boundaries(b, acc, c_one, z, z);
  return b.fold(acc, b.emit(kMul, b.extra(kXActive),
                            b.emit(kSub, b.emit(kMul, b.extra(kXGroup, 1), value), b.emit(kMul, z, input_value))));
}

// ---------------------------------------------------------------------------
// Lowering

enum LKind : uint32_t { kLConst = 0, kLSlot, kLSpill, kLColumn, kLAcc, kLXRow, kLOut };
enum LOp : uint32_t { kLAdd = 0, kLSub, kLMul, kLSquare, kLDouble, kLNegate, kLCopy };

// One instruction of the kernel's stream: dst = op(a, b).  A column operand's
// index counts [fixed | advice | instance | extra] and its rot is already in
// [0, n); a constant's counts [graph constants | challenges | beta gamma
// theta y]; a slot's is its LDS slot, a spill's its row of the workspace.
struct LInstr {
  uint32_t op, dst_kind, dst;
  uint32_t a_kind, a, a_rot;
  uint32_t b_kind, b, b_rot;
  uint32_t pad[3];
};
static_assert(sizeof(LInstr) == 48, "LInstr: twelve words");

struct Program {
  std::vector<LInstr> code;
  size_t slots_needed = 0;  // fast and spilled together
  size_t spill_slots = 0;   // those beyond fast_slots
  size_t num_consts = 0;    // the constant table's length
  size_t products = 0;      // Mul and Square instructions (field products per row)
  size_t column_reads = 0;  // column operands (elements read per row)
  bool uses_xrow = false;
};

inline size_t const_table_size(const Graph& g, const Sizes& t) { return g.num_constants + t.num_challenges + 4; }

namespace detail {
struct VOperand {
  uint32_t kind;  // an LKind, or kValue
  uint32_t index, rot;
};
inline constexpr uint32_t kValue = 100;
struct VInstr {
  uint32_t op;
  uint32_t dst;  // value id
  VOperand a, b;
};
}  // namespace detail

// g: validated against t (graph_ok); result: the source whose value goes to
// the accumulator; n: the rows (rotations are reduced modulo n).
inline Program lower(const Graph& g, const Sizes& t, Source result, size_t n, size_t fast_slots) {
  using namespace detail;
  std::vector<VInstr> v;
  std::vector<VOperand> cur(g.num_intermediates, VOperand{kLConst, 0, 0});
  uint32_t num_values = 0;
  auto operand = [&](const Source& s) -> VOperand {
    switch (s.kind) {
      case kConstant: return {kLConst, s.index, 0};
      case kIntermediate: return cur[s.index];
      case kFixed:
      case kAdvice:
      case kInstance:
      case kExtra: {
        const uint32_t base = s.kind == kFixed      ? 0
                              : s.kind == kAdvice   ? (uint32_t)t.num_fixed
                              : s.kind == kInstance ? (uint32_t)(t.num_fixed + t.num_advice)
                                                    : (uint32_t)(t.num_fixed + t.num_advice + t.num_instance);
        const int64_t m = (int64_t)n, r = ((int64_t)g.rotations[s.rotation_index] % m + m) % m;
        return {kLColumn, base + s.index, (uint32_t)r};
      }
      case kChallenge: return {kLConst, (uint32_t)g.num_constants + s.index, 0};
      case kBeta:
      case kGamma:
      case kTheta:
      case kY: return {kLConst, (uint32_t)(g.num_constants + t.num_challenges) + (s.kind - kBeta), 0};
      case kXRow: return {kLXRow, 0, 0};
      default: return {kLAcc, 0, 0};  // kPreviousValue, kAcc
    }
  };
  auto emit = [&](uint32_t op, VOperand a, VOperand b) -> VOperand {
    v.push_back({op, num_values, a, b});
    return {kValue, num_values++, 0};
  };
  const VOperand none{kLConst, 0, 0};
  for (size_t i = 0; i < g.num_calcs; ++i) {
    const Calc& c = g.calcs[i];
    VOperand r;
    switch (c.op) {
      case kAdd: r = emit(kLAdd, operand(c.a), operand(c.b)); break;
      case kSub: r = emit(kLSub, operand(c.a), operand(c.b)); break;
      case kMul: r = emit(kLMul, operand(c.a), operand(c.b)); break;
      case kSquare: r = emit(kLSquare, operand(c.a), none); break;
      case kDouble: r = emit(kLDouble, operand(c.a), none); break;
      case kNegate: r = emit(kLNegate, operand(c.a), none); break;
      case kStore: r = operand(c.a); break;  // an alias, not a copy
      default: {                             // Horner: v = init; v = v factor + part
        r = operand(c.a);
        const VOperand factor = operand(c.b);
        for (uint32_t k = 0; k < c.parts_count; ++k)
          r = emit(kLAdd, emit(kLMul, r, factor), operand(g.parts[c.parts_begin + k]));
      }
    }
    cur[c.target] = r;
  }
  const VOperand res = operand(result);
  // the accumulator's new value: the last instruction writes it, or a copy does
  const bool direct = res.kind == kValue && !v.empty() && v.back().dst == res.index;
  if (!direct) v.push_back({kLCopy, UINT32_MAX, res, none});

  // last use of every value
  std::vector<size_t> last(num_values);
  for (size_t i = 0; i < v.size(); ++i) {
    if (v[i].dst != UINT32_MAX) last[v[i].dst] = i;
    if (v[i].a.kind == kValue) last[v[i].a.index] = i;
    if (v[i].b.kind == kValue) last[v[i].b.index] = i;
  }
  Program p;
  p.num_consts = const_table_size(g, t);
  std::vector<uint32_t> slot_of(num_values, 0);
  std::vector<char> busy;
  auto place = [&](const VOperand& o, uint32_t* kind, uint32_t* index, uint32_t* rot) {
    *kind = o.kind, *index = o.index, *rot = o.rot;
    if (o.kind == kValue) {
      const uint32_t s = slot_of[o.index];
      *kind = s < fast_slots ? kLSlot : kLSpill;
      *index = s < fast_slots ? s : s - (uint32_t)fast_slots;
    }
    p.column_reads += o.kind == kLColumn;
    p.uses_xrow |= o.kind == kLXRow;
  };
  for (size_t i = 0; i < v.size(); ++i) {
    LInstr ins{};
    ins.op = v[i].op;
    place(v[i].a, &ins.a_kind, &ins.a, &ins.a_rot);
    const bool two = ins.op == kLAdd || ins.op == kLSub || ins.op == kLMul;
    if (two) place(v[i].b, &ins.b_kind, &ins.b, &ins.b_rot);
    p.products += ins.op == kLMul || ins.op == kLSquare;
    // operands that die here give their slots up before the result takes one:
    // the kernel reads both operands before it writes
    for (const VOperand* o : {&v[i].a, &v[i].b})
      if (o->kind == kValue && (o == &v[i].a || two) && last[o->index] == i) busy[slot_of[o->index]] = 0;
    const bool is_result = i + 1 == v.size();
    if (is_result) {
      ins.dst_kind = kLOut;
    } else {
      size_t s = 0;
      while (s < busy.size() && busy[s]) ++s;
      if (s == busy.size()) busy.push_back(0);
      busy[s] = 1;
      slot_of[v[i].dst] = (uint32_t)s;
      ins.dst_kind = s < fast_slots ? kLSlot : kLSpill;
      ins.dst = (uint32_t)(s < fast_slots ? s : s - fast_slots);
      if (last[v[i].dst] == i) busy[s] = 0;  // never read: the slot is free again at once
    }
    p.code.push_back(ins);
  }
  p.slots_needed = busy.size();
  p.spill_slots = p.slots_needed > fast_slots ? p.slots_needed - fast_slots : 0;
  return p;
}

// One row of a lowered program over the field F (+, -, *, and F() = 0).
// consts: the constant table; column(c, r): row r of column c; acc: the
// accumulator's value on this row; xrow: the label on this row.  Returns the
// accumulator's new value.
template <class F, class ColumnFn>
F run_row(const Program& p, size_t fast_slots, const F* consts, ColumnFn&& column, size_t row, size_t n, const F& acc,
          const F& xrow) {
  std::vector<F> slots(p.slots_needed);
  F out = F();
  auto read = [&](uint32_t kind, uint32_t index, uint32_t rot) -> F {
    switch (kind) {
      case kLConst: return consts[index];
      case kLSlot: return slots[index];
      case kLSpill: return slots[fast_slots + index];
      case kLColumn: return column(index, (row + rot) % n);
      case kLAcc: return acc;
      default: return xrow;
    }
  };
  for (const LInstr& ins : p.code) {
    const F a = read(ins.a_kind, ins.a, ins.a_rot);
    F r;
    switch (ins.op) {
      case kLAdd: r = a + read(ins.b_kind, ins.b, ins.b_rot); break;
      case kLSub: r = a - read(ins.b_kind, ins.b, ins.b_rot); break;
      case kLMul: r = a * read(ins.b_kind, ins.b, ins.b_rot); break;
      case kLSquare: r = a * a; break;
      case kLDouble: r = a + a; break;
      case kLNegate: r = F() - a; break;
      default: r = a;
    }
    if (ins.dst_kind == kLOut) out = r;
    else slots[ins.dst_kind == kLSlot ? ins.dst : fast_slots + ins.dst] = r;
  }
  return out;
}

}  // namespace tachyon_amd::quotient_plan
