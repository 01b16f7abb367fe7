// Host-only check of plonk/quotient_plan.h (no library, no HIP): every
// refusal of the quotient entry points is refused, and over a 61-bit prime
// toy field run_row(lower(g)) equals a direct walk of the graph (the
// reference's rule: graph_evaluator.h:60-76, calculation.h:71-104) on random
// graphs, a graph whose live set is 1, one whose intermediates all stay live,
// Horner of 0 and 1 part, with slots_needed the largest live count; the
// closed forms the Builder writes equal their formulas.  Not part of `all`:
//   make ../bin/quotient_plan_check [CXX=... HOST_CHECK_FLAGS=-fsanitize=address,undefined]
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../plonk/quotient_plan.h"

namespace {

using namespace tachyon_amd::quotient_plan;

constexpr uint64_t kP = (uint64_t(1) << 61) - 1;
struct F {
  uint64_t v = 0;
  F() = default;
  explicit F(uint64_t x) : v(x % kP) {}
  F operator+(const F& o) const { return F(v + o.v); }
  F operator-(const F& o) const { return F(v + kP - o.v); }
  F operator*(const F& o) const { return F((uint64_t)((unsigned __int128)v * o.v % kP)); }
  bool operator==(const F& o) const { return v == o.v; }
};

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    printf("FAIL: %s\n", what);
    ++failures;
  }
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}

// A table of columns over n rows and the uniform values
struct World {
  size_t n = 8;
  Sizes sizes;
  std::vector<std::vector<F>> cols;  // [fixed | advice | instance | extra]
  std::vector<F> challenges;
  F beta, gamma, theta, y;
  explicit World(size_t rows, size_t nf = 2, size_t na = 3, size_t ni = 1, size_t nc = 2, size_t nx = 0) : n(rows) {
    sizes = {nf, na, ni, nc, nx, nx != 0};
    cols.assign(nf + na + ni + nx, std::vector<F>(n));
    for (auto& c : cols)
      for (F& x : c) x = F(rnd());
    for (size_t i = 0; i < nc; ++i) challenges.push_back(F(rnd()));
    beta = F(rnd()), gamma = F(rnd()), theta = F(rnd()), y = F(rnd());
  }
  size_t base(uint32_t kind) const {
    return kind == kFixed ? 0 : kind == kAdvice ? sizes.num_fixed : kind == kInstance ? sizes.num_fixed + sizes.num_advice
                                                                                      : sizes.num_fixed + sizes.num_advice + sizes.num_instance;
  }
  F at(uint32_t kind, uint32_t index, int64_t row) const {
    const int64_t m = (int64_t)n;
    return cols[base(kind) + index][(size_t)(((row % m) + m) % m)];
  }
};

// The graph's value on a row, walked the reference's way
F walk(const Graph& g, const F* constants, const World& w, size_t row, const F& prev, const F& xrow) {
  std::vector<F> inter(g.num_intermediates);
  auto get = [&](const Source& s) -> F {
    switch (s.kind) {
      case kConstant: return constants[s.index];
      case kIntermediate: return inter[s.index];
      case kFixed:
      case kAdvice:
      case kInstance:
      case kExtra: return w.at(s.kind, s.index, (int64_t)row + g.rotations[s.rotation_index]);
      case kChallenge: return w.challenges[s.index];
      case kBeta: return w.beta;
      case kGamma: return w.gamma;
      case kTheta: return w.theta;
      case kY: return w.y;
      case kXRow: return xrow;
      default: return prev;
    }
  };
  for (size_t i = 0; i < g.num_calcs; ++i) {
    const Calc& c = g.calcs[i];
    F r;
    switch (c.op) {
      case kAdd: r = get(c.a) + get(c.b); break;
      case kSub: r = get(c.a) - get(c.b); break;
      case kMul: r = get(c.a) * get(c.b); break;
      case kSquare: r = get(c.a) * get(c.a); break;
      case kDouble: r = get(c.a) + get(c.a); break;
      case kNegate: r = F() - get(c.a); break;
      case kStore: r = get(c.a); break;
      default: {
        const F factor = get(c.b);
        r = get(c.a);
        for (uint32_t k = 0; k < c.parts_count; ++k) r = r * factor + get(g.parts[c.parts_begin + k]);
      }
    }
    inter[c.target] = r;
  }
  return g.num_calcs ? inter[g.calcs[g.num_calcs - 1].target] : F();
}

std::vector<F> const_table(const Graph& g, const F* constants, const World& w) {
  std::vector<F> t(constants, constants + g.num_constants);
  t.insert(t.end(), w.challenges.begin(), w.challenges.end());
  for (const F& x : {w.beta, w.gamma, w.theta, w.y}) t.push_back(x);
  return t;
}

// The most slots a program holds at once, recounted from its instructions
// alone: a value holds its slot from the instruction that writes it up to the
// one before its last read (operands give their slots up before the result
// takes one), or for its own instruction when nothing reads it.
size_t max_occupied(const Program& p, size_t fast) {
  auto loc = [&](uint32_t kind, uint32_t index) -> long {
    return kind == kLSlot ? (long)index : kind == kLSpill ? (long)(fast + index) : -1;
  };
  std::vector<long> def(p.slots_needed, -1), last(p.slots_needed, -1), delta(p.code.size() + 2, 0);
  auto close = [&](long l) {
    if (def[l] < 0) return;
    delta[def[l]] += 1;
    delta[(last[l] > def[l] ? last[l] - 1 : def[l]) + 1] -= 1;
  };
  for (size_t i = 0; i < p.code.size(); ++i) {
    const LInstr& ins = p.code[i];
    const long a = loc(ins.a_kind, ins.a), b = ins.op <= kLMul ? loc(ins.b_kind, ins.b) : -1;
    if (a >= 0) last[a] = (long)i;
    if (b >= 0) last[b] = (long)i;
    const long d = loc(ins.dst_kind, ins.dst);
    if (d >= 0) {
      close(d);
      def[d] = (long)i, last[d] = -1;
    }
  }
  for (size_t l = 0; l < p.slots_needed; ++l) close((long)l);
  long live = 0, most = 0;
  for (size_t i = 0; i < p.code.size(); ++i) most = std::max(most, live += delta[i]);
  return (size_t)most;
}

// run_row(lower(g)) against walk on every row, for several LDS slot counts
void same_meaning(const Graph& g, const F* constants, const World& w, Source result, const char* what,
                  size_t* slots_needed = nullptr) {
  expect(graph_ok(g, w.sizes), what);
  const std::vector<F> table = const_table(g, constants, w);
  for (size_t fast : {size_t(0), size_t(1), size_t(3), size_t(1000)}) {
    const Program p = lower(g, w.sizes, result, w.n, fast);
    expect(p.num_consts == table.size(), "constant table size");
    expect(p.slots_needed == max_occupied(p, fast), "slots_needed is the largest live count");
    expect(p.spill_slots == (p.slots_needed > fast ? p.slots_needed - fast : 0), "spill count");
    for (const LInstr& ins : p.code) {
      expect(ins.dst_kind == kLOut || (ins.dst_kind == kLSlot ? ins.dst < fast : ins.dst < p.spill_slots), "slot bounds");
      expect(ins.a_kind != kLColumn || ins.a_rot < w.n, "rotation reduced");
    }
    if (slots_needed) *slots_needed = p.slots_needed;
    for (size_t row = 0; row < w.n; ++row) {
      const F prev(rnd()), xrow(rnd());
      const F want = result.kind == kIntermediate || g.num_calcs == 0 ? walk(g, constants, w, row, prev, xrow) : prev;
      const F got = run_row<F>(
          p, fast, table.data(), [&](uint32_t c, size_t r) { return w.cols[c][r]; }, row, w.n, prev, xrow);
      expect(got == want, what);
    }
  }
}

Source last_of(const std::vector<Calc>& calcs) {
  return calcs.empty() ? Source{kConstant, 0, 0} : Source{kIntermediate, calcs.back().target, 0};
}

struct OwnedGraph {
  std::vector<Calc> calcs;
  std::vector<Source> parts;
  std::vector<F> constants{F(0), F(1), F(2)};
  std::vector<int32_t> rotations{0};
  size_t num_intermediates = 0;
  Graph view() const {
    return {calcs.data(),     calcs.size(),     parts.data(), parts.size(), constants.data(), constants.size(),
            rotations.data(), rotations.size(), num_intermediates};
  }
};

OwnedGraph random_graph(const World& w, size_t num_calcs, bool reuse_targets) {
  OwnedGraph g;
  g.rotations = {0, 1, -1, 5, (int32_t)w.n + 3, -(int32_t)w.n - 3};
  for (int i = 0; i < 4; ++i) g.constants.push_back(F(rnd()));
  g.num_intermediates = num_calcs;
  std::vector<uint32_t> written;
  auto source = [&]() -> Source {
    for (;;) {
      const uint32_t kind = (uint32_t)(rnd() % kPublicKinds);
      const uint32_t rot = (uint32_t)(rnd() % g.rotations.size());
      switch (kind) {
        case kConstant: return {kind, (uint32_t)(rnd() % g.constants.size()), 0};
        case kIntermediate:
          if (written.empty()) continue;
          return {kind, written[rnd() % written.size()], 0};
        case kFixed: return {kind, (uint32_t)(rnd() % w.sizes.num_fixed), rot};
        case kAdvice: return {kind, (uint32_t)(rnd() % w.sizes.num_advice), rot};
        case kInstance: return {kind, (uint32_t)(rnd() % w.sizes.num_instance), rot};
        case kChallenge: return {kind, (uint32_t)(rnd() % w.sizes.num_challenges), 0};
        default: return {kind, 0, 0};
      }
    }
  };
  for (size_t i = 0; i < num_calcs; ++i) {
    Calc c{};
    c.op = (uint32_t)(rnd() % kNumOps);
    c.a = source();
    c.b = source();
    if (c.op == kHorner) {
      c.parts_begin = (uint32_t)g.parts.size();
      c.parts_count = (uint32_t)(rnd() % 4);
      for (uint32_t k = 0; k < c.parts_count; ++k) g.parts.push_back(source());
    }
    c.target = reuse_targets && !written.empty() && rnd() % 4 == 0 ? written[rnd() % written.size()] : (uint32_t)i;
    g.calcs.push_back(c);
    written.push_back(c.target);
  }
  return g;
}

void check_lowering() {
  const World w(8);
  for (int round = 0; round < 200; ++round) {
    const OwnedGraph g = random_graph(w, 1 + rnd() % 40, round % 2 == 1);
    same_meaning(g.view(), g.constants.data(), w, last_of(g.calcs), "random graph");
  }
  {  // no calculation: zero
    OwnedGraph g;
    same_meaning(g.view(), g.constants.data(), w, Source{kConstant, 0, 0}, "empty graph");
  }
  {  // every value dies in the next calculation: one slot
    OwnedGraph g;
    const Source col{kAdvice, 1, 0};
    for (uint32_t i = 0; i < 30; ++i) {
      const Source prev = i ? Source{kIntermediate, i - 1, 0} : col;
      g.calcs.push_back({i % 3 == 0 ? (uint32_t)kAdd : i % 3 == 1 ? (uint32_t)kMul : (uint32_t)kSquare, prev, col, 0, 0, i});
    }
    g.num_intermediates = 30;
    size_t slots = 0;
    same_meaning(g.view(), g.constants.data(), w, last_of(g.calcs), "chain", &slots);
    expect(slots == 1, "a chain needs one slot");
  }
  {  // K values all read by the last calculation: K slots and the Horner's running value
    OwnedGraph g;
    const uint32_t K = 25;
    for (uint32_t i = 0; i < K; ++i) {
      g.calcs.push_back({kAdd, Source{kAdvice, i % 3, 0}, Source{kConstant, 3 + i % 4, 0}, 0, 0, i});
      g.constants.push_back(F(rnd()));
      g.parts.push_back(Source{kIntermediate, i, 0});
    }
    g.calcs.push_back({kHorner, Source{kConstant, 0, 0}, Source{kTheta, 0, 0}, 0, K, K});
    g.num_intermediates = K + 1;
    size_t slots = 0;
    same_meaning(g.view(), g.constants.data(), w, last_of(g.calcs), "all live", &slots);
    expect(slots == K + 1, "all live: every value and the running one");
  }
  for (uint32_t count : {0u, 1u}) {  // Horner of no part (its initial value) and of one
    for (uint32_t init : {(uint32_t)kPreviousValue, (uint32_t)kConstant}) {
      OwnedGraph g;
      g.parts.push_back(Source{kFixed, 1, 0});
      g.calcs.push_back({kHorner, Source{init, 0, 0}, Source{init == kConstant ? (uint32_t)kTheta : (uint32_t)kY, 0, 0}, 0, count, 0});
      g.num_intermediates = 1;
      same_meaning(g.view(), g.constants.data(), w, last_of(g.calcs), "short Horner");
    }
  }
  {  // a Store is an alias: a column stored, rotated, and read twice costs no slot
    OwnedGraph g;
    g.rotations = {0, -1};
    g.calcs.push_back({kStore, Source{kFixed, 0, 1}, Source{}, 0, 0, 0});
    g.calcs.push_back({kMul, Source{kIntermediate, 0, 0}, Source{kIntermediate, 0, 0}, 0, 0, 1});
    g.num_intermediates = 2;
    size_t slots = 9;
    same_meaning(g.view(), g.constants.data(), w, last_of(g.calcs), "store alias", &slots);
    expect(slots == 0, "a stored column takes no slot");
  }
}

// The closed forms against their formulas (permutation_evaluator.h:25-108,
// lookup/halo2/evaluator.h:66-128, shuffle/evaluator.h:71-119)
void check_closed_forms() {
  const size_t n = 16;
  const F one(1), zero(0);
  for (size_t L : {size_t(1), size_t(2), size_t(7)}) {
    for (size_t m : {size_t(0), L, L + 1, 2 * L + 1}) {
      const size_t k = (m + L - 1) / L;
      World w(n, 2, 3, 1, 1, 3 + k + m);
      std::vector<Source> cols;
      for (size_t i = 0; i < m; ++i) cols.push_back({i % 3 == 0 ? (uint32_t)kFixed : i % 3 == 1 ? (uint32_t)kAdvice : (uint32_t)kInstance, (uint32_t)(i % 3 == 1 ? i % 3 : 0), 0});
      const F delta(rnd());
      std::vector<F> dp(m ? m : 1, one);
      for (size_t i = 1; i < m; ++i) dp[i] = dp[i - 1] * delta;
      std::vector<const void*> dptr;
      for (const F& d : dp) dptr.push_back(&d);
      Builder b;
      b.elem_bytes = sizeof(F);
      const int32_t last_row = -4;
      const Source res = build_permutation(b, Source{kAcc, 0, 0}, &one, cols.data(), m, L, last_row, dptr.data());
      std::vector<F> consts;
      for (const void* c : b.constants) consts.push_back(*static_cast<const F*>(c));
      const Graph g = b.view();
      expect(graph_ok(g, w.sizes), "permutation graph valid");
      const Program p = lower(g, w.sizes, res, n, 4);
      const std::vector<F> table = const_table(g, consts.data(), w);
      for (size_t row = 0; row < n; ++row) {
        const F prev(rnd()), xrow(rnd());
        auto X = [&](size_t i, int64_t rot = 0) { return w.at(kExtra, (uint32_t)i, (int64_t)row + rot); };
        F acc = prev;
        if (m) {
          acc = acc * w.y + (one - X(3)) * X(0);
          acc = acc * w.y + X(1) * (X(3 + k - 1) * X(3 + k - 1) - X(3 + k - 1));
          for (size_t j = 1; j < k; ++j) acc = acc * w.y + X(0) * (X(3 + j) - X(3 + j - 1, last_row));
          F cur = xrow;
          for (size_t j = 0; j < k; ++j) {
            F left = X(3 + j, 1), right = X(3 + j);
            for (size_t i = j * L; i < std::min(m, (j + 1) * L); ++i) {
              const F v = w.at(cols[i].kind, cols[i].index, (int64_t)row);
              left = left * (v + w.beta * X(3 + k + i) + w.gamma);
              right = right * (v + cur + w.gamma);
              cur = cur * delta;
            }
            acc = acc * w.y + (left - right) * X(2);
          }
        }
        const F got = run_row<F>(
            p, 4, table.data(), [&](uint32_t c, size_t r) { return w.cols[c][r]; }, row, n, prev, xrow);
        expect(got == acc, "permutation closed form");
      }
    }
  }
  // lookup and shuffle around random compressed-expression graphs
  for (int round = 0; round < 20; ++round) {
    World w(n, 2, 3, 1, 2, 6);
    const OwnedGraph g1 = random_graph(w, round % 5 == 0 ? 0 : 1 + rnd() % 12, false);
    const OwnedGraph g2 = random_graph(w, 1 + rnd() % 12, false);
    for (int shuffle = 0; shuffle < 2; ++shuffle) {
      Builder b;
      b.elem_bytes = sizeof(F);
      const Graph v1 = g1.view(), v2 = g2.view();
      const Source res = shuffle ? build_shuffle(b, Source{kAcc, 0, 0}, &one, &zero, v1, v2)
                                 : build_lookup(b, Source{kAcc, 0, 0}, &one, &zero, v1);
      std::vector<F> consts;
      for (const void* c : b.constants) consts.push_back(*static_cast<const F*>(c));
      const Graph g = b.view();
      expect(graph_ok(g, w.sizes), "closed-form graph valid");
      const Program p = lower(g, w.sizes, res, n, 4);
      const std::vector<F> table = const_table(g, consts.data(), w);
      for (size_t row = 0; row < n; ++row) {
        const F prev(rnd()), xrow(rnd());
        auto X = [&](size_t i, int64_t rot = 0) { return w.at(kExtra, (uint32_t)i, (int64_t)row + rot); };
        const F t1 = walk(v1, g1.constants.data(), w, row, zero, xrow), t2 = walk(v2, g2.constants.data(), w, row, zero, xrow);
        F acc = prev;
        acc = acc * w.y + X(0) * (one - X(3));
        acc = acc * w.y + X(1) * (X(3) * X(3) - X(3));
        if (shuffle) {
          acc = acc * w.y + X(2) * (X(3, 1) * t2 - X(3) * t1);
        } else {
          const F ams = X(4) - X(5);
          acc = acc * w.y + X(2) * (X(3, 1) * (X(4) + w.beta) * (X(5) + w.gamma) - X(3) * t1);
          acc = acc * w.y + X(0) * ams;
          acc = acc * w.y + X(2) * ams * (X(4) - X(4, -1));
        }
        const F got = run_row<F>(
            p, 4, table.data(), [&](uint32_t c, size_t r) { return w.cols[c][r]; }, row, n, prev, xrow);
        expect(got == acc, shuffle ? "shuffle closed form" : "lookup closed form");
      }
    }
  }
}

// One valid evaluate_part / h_poly call whose pieces each refusal damages.
// Columns are one element long: the checks never read one.
struct Call {
  unsigned char elem[32] = {1};
  const void* col = elem;
  const void* fixed[2] = {elem, elem};
  const void* advice[1] = {elem};
  const void* instance[1] = {elem};
  const void* zs[2] = {elem, elem};
  const void* sigmas[3] = {elem, elem, elem};
  unsigned char constants[3 * 32] = {};
  int32_t rotations[2] = {0, -1};
  Source parts[2] = {{kFixed, 1, 1}, {kChallenge, 0, 0}};
  Calc calcs[3] = {{kStore, {kAdvice, 0, 1}, {}, 0, 0, 0},
                   {kMul, {kIntermediate, 0, 0}, {kConstant, 2, 0}, 0, 0, 1},
                   {kHorner, {kPreviousValue, 0, 0}, {kY, 0, 0}, 0, 2, 2}};
  Graph graph{calcs, 3, parts, 2, constants, 3, rotations, 2, 3};
  Source perm_cols[3] = {{kFixed, 1, 0}, {kAdvice, 0, 0}, {kInstance, 0, 0}};
  Table table{fixed, 2, advice, 1, instance, 1, elem, 1};
  Params params{0, 8, 4, -3, elem, elem, elem, elem, elem, elem, elem};
  Group group{kGates, &graph, &graph, zs, 1, elem, elem, perm_cols, 3, sigmas, elem, elem, elem};
  System system{&graph, perm_cols, 3, sigmas, &graph, 1, nullptr, 0};
  Graph shuffles[2];
  Circuit circuit{};
  const void* zeta = elem;
  const void* delta = elem;
  void* out = elem;
  uint32_t two_adicity = 28;
  Call() {
    shuffles[0] = shuffles[1] = graph;
    system.shuffles = shuffles;
    system.num_shuffles = 1;
    circuit = {table, zs, 2, zs, zs, zs, zs};
  }
  bool part() const { return part_ok(&params, &table, &group, elem, two_adicity); }
  bool h() const { return h_poly_ok(&params, &system, &circuit, 1, zeta, delta, out, two_adicity); }
};

void refused(const char* what, const std::function<void(Call&)>& damage, bool part = true, bool h = true) {
  Call c;
  damage(c);
  if (part) expect(!c.part(), what);
  if (h) expect(!c.h(), what);
}

void check_refusals() {
  {
    Call c;
    expect(c.part() && c.h(), "a valid call passes");
    for (uint32_t kind : {kPermutation, kLookup, kShuffle}) {
      Call d;
      d.group.kind = kind;
      d.group.num_z = kind == kPermutation ? 2 : 1;
      expect(d.part(), "a valid closed-form group passes");
    }
  }
  refused("source kind out of range", [](Call& c) { c.calcs[0].a.kind = kPublicKinds; });
  refused("an internal kind from outside", [](Call& c) { c.calcs[0].a.kind = kAcc; });
  refused("op out of range", [](Call& c) { c.calcs[1].op = kNumOps; });
  refused("constant index", [](Call& c) { c.calcs[1].b.index = 3; });
  refused("fixed column index", [](Call& c) { c.parts[0].index = 2; });
  refused("advice column index", [](Call& c) { c.calcs[0].a.index = 1; });
  refused("instance column index", [](Call& c) { c.calcs[0].a = {kInstance, 1, 0}; });
  refused("rotation index", [](Call& c) { c.calcs[0].a.rotation_index = 2; });
  refused("challenge index", [](Call& c) { c.parts[1].index = 1; });
  refused("Horner parts past the end", [](Call& c) { c.calcs[2].parts_count = 3; });
  refused("Horner parts begin past the end", [](Call& c) { c.calcs[2].parts_begin = 3, c.calcs[2].parts_count = 0; });
  refused("Horner parts overflow", [](Call& c) { c.calcs[2].parts_begin = 2, c.calcs[2].parts_count = UINT32_MAX; });
  refused("target out of range", [](Call& c) { c.calcs[2].target = 3; });
  refused("intermediate read before it is written", [](Call& c) { c.calcs[1].a.index = 2; });
  refused("intermediate read by its own calculation", [](Call& c) { c.calcs[1].a.index = 1; });
  refused("intermediate index", [](Call& c) { c.calcs[1].a.index = 7; });
  refused("n not a power of two", [](Call& c) { c.params.n = 12; });
  refused("n < 2", [](Call& c) { c.params.n = 1; });
  refused("n = 0", [](Call& c) { c.params.n = 0; });
  refused("cs_degree < 3", [](Call& c) { c.params.cs_degree = 2; });
  refused("field", [](Call& c) { c.params.field = 1; });
  refused("two-adicity", [](Call& c) { c.params.n = size_t(1) << 27, c.params.cs_degree = 4; }, false, true);
  {
    Call c;
    c.params.n = size_t(1) << 26, c.params.cs_degree = 4;
    expect(c.h(), "the largest extended domain passes");
  }
  refused("null calcs", [](Call& c) { c.graph.calcs = nullptr; });
  refused("null parts", [](Call& c) { c.graph.parts = nullptr; });
  refused("null constants", [](Call& c) { c.graph.constants = nullptr; });
  refused("null rotations", [](Call& c) { c.graph.rotations = nullptr; });
  refused("null theta", [](Call& c) { c.params.theta = nullptr; });
  refused("null y", [](Call& c) { c.params.y = nullptr; });
  refused("null column", [](Call& c) { c.fixed[1] = nullptr; });
  refused("null column array", [](Call& c) { c.table.advice = nullptr, c.circuit.table.advice = nullptr; });
  refused("null challenges", [](Call& c) { c.table.challenges = nullptr, c.circuit.table.challenges = nullptr; });
  refused("null graph", [](Call& c) { c.group.graph = nullptr; }, true, false);
  refused("null zeta", [](Call& c) { c.zeta = nullptr; }, false, true);
  refused("null delta with a permutation", [](Call& c) { c.delta = nullptr; }, false, true);
  refused("null out", [](Call& c) { c.out = nullptr; }, false, true);
  refused("null l_first", [](Call& c) { c.params.l_first = nullptr, c.group.kind = kLookup; });
  refused("null lookup z", [](Call& c) { c.circuit.lookup_z = nullptr; }, false, true);
  refused("null shuffle z", [](Call& c) { c.zs[1] = nullptr, c.zs[0] = nullptr; }, false, true);
  refused("group kind", [](Call& c) { c.group.kind = kNumGroups; }, true, false);
  refused("permutation column names no column", [](Call& c) { c.group.kind = kPermutation, c.group.num_z = 2, c.perm_cols[1].index = 1; });
  refused("permutation column of another kind", [](Call& c) { c.group.kind = kPermutation, c.group.num_z = 2, c.perm_cols[0].kind = kChallenge; });
  refused("z count below ceil(m / (cs_degree - 2))", [](Call& c) { c.group.kind = kPermutation, c.group.num_z = 1, c.circuit.num_perm_z = 1; });
  refused("z count above", [](Call& c) { c.group.kind = kPermutation, c.group.num_z = 3, c.circuit.num_perm_z = 3; });
  refused("null sigma", [](Call& c) { c.group.kind = kPermutation, c.group.num_z = 2, c.sigmas[2] = nullptr; });
  refused("null x_scale", [](Call& c) { c.group.kind = kPermutation, c.group.num_z = 2, c.group.x_scale = nullptr; }, true, false);
  refused("lookup without a permuted input", [](Call& c) { c.group.kind = kLookup, c.group.a_perm = nullptr; }, true, false);
  refused("shuffle without its second graph", [](Call& c) { c.group.kind = kShuffle, c.group.graph2 = nullptr; }, true, false);
  expect(extended_log(16, 3) == 5 && extended_log(16, 4) == 6 && extended_log(16, 5) == 6 && extended_log(16, 9) == 7,
         "extended_k");
  expect(perm_z_count(0, 3) == 0 && perm_z_count(3, 4) == 2 && perm_z_count(15, 9) == 3, "z count");
}

}  // namespace

int main() {
  check_refusals();
  check_lowering();
  check_closed_forms();
  if (failures) return printf("%d failure(s)\n", failures), 1;
  puts("quotient_plan_check ok");
  return 0;
}
