// Grouping and argument checks of the KZG opening entry points
// (include/tachyon_mi355x.h, tachyon_mi355x_kzg_opening_plan /
// _create_opening_proof): host-only C++ with no HIP dependency, so the grouping
// and the refusal rules can be compiled and run on their own.
//
// Reference: tachyon/crypto/commitments/polynomial_openings.h
//   GroupBySinglePoint (GWC, :191-213): one group per distinct point in order
//     of first appearance, every opening at it kept (duplicates too);
//   GroupByPolyOracleAndPoints (SHPlonk, :216-240): each polynomial's SET of
//     points, then one group per distinct set in order of first appearance,
//     the claimed value of (polynomial, point) being the first opening's.
// A polynomial's identity is its index (the reference's shallow Ref); a
// group's points and the super point set are ordered by the field's
// operator< (absl::btree_set<Point>), supplied by the caller as `less` over
// the elements' bytes; equal elements have equal bytes (canonical Montgomery
// form).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tachyon_amd::kzg_open {

inline constexpr int kGwc = 0;
inline constexpr int kShplonk = 1;

// Openings are referred to by their index in the caller's list: a group's
// point is the index of the first opening at that point, a claimed value the
// index of the opening that carries it.
struct Group {
  std::vector<size_t> points;
  std::vector<size_t> polys;
  // values[j * points.size() + k]: the opening of polys[j] at points[k]
  std::vector<size_t> values;
};

struct Plan {
  std::vector<Group> groups;
  std::vector<size_t> super_points;  // every distinct point, ordered
};

struct Openings {
  const size_t* poly = nullptr;            // count polynomial indices
  const unsigned char* points = nullptr;   // count elements of elem_bytes
  const unsigned char* values = nullptr;   // count elements of elem_bytes
  size_t elem_bytes = 32;
  size_t count = 0;

  const unsigned char* point(size_t i) const { return points + i * elem_bytes; }
  const unsigned char* value(size_t i) const { return values + i * elem_bytes; }
  bool same_point(size_t a, size_t b) const { return memcmp(point(a), point(b), elem_bytes) == 0; }
  bool same_value(size_t a, size_t b) const { return memcmp(value(a), value(b), elem_bytes) == 0; }
};

inline bool scheme_ok(int scheme) { return scheme == kGwc || scheme == kShplonk; }

// The refusals that need no grouping: a null array with a nonzero count, an
// index out of range, a polynomial longer than the SRS.  lens may be null
// only when there are no polynomials.
inline bool arguments_ok(const Openings& o, const size_t* lens, size_t num_polys, size_t n) {
  if (o.count != 0 && (!o.poly || !o.points || !o.values)) return false;
  if (num_polys != 0 && !lens) return false;
  for (size_t i = 0; i < num_polys; ++i)
    if (lens[i] > n) return false;
  for (size_t i = 0; i < o.count; ++i)
    if (o.poly[i] >= num_polys) return false;
  return true;
}

// Index of the first opening whose point equals opening i's
inline size_t first_at_point(const Openings& o, size_t i) {
  for (size_t j = 0; j < i; ++j)
    if (o.same_point(j, i)) return j;
  return i;
}

template <class Less>
void sort_points(const Openings& o, Less less, std::vector<size_t>* pts) {
  std::sort(pts->begin(), pts->end(), [&](size_t a, size_t b) { return less(o.point(a), o.point(b)); });
}

template <class Less>
void group_by_single_point(const Openings& o, Less less, Plan* plan) {
  plan->groups.clear();
  plan->super_points.clear();
  for (size_t i = 0; i < o.count; ++i) {
    const size_t pt = first_at_point(o, i);
    auto it = std::find_if(plan->groups.begin(), plan->groups.end(), [&](const Group& g) { return g.points[0] == pt; });
    if (it == plan->groups.end()) {
      plan->groups.push_back(Group{{pt}, {}, {}});
      plan->super_points.push_back(pt);
      it = plan->groups.end() - 1;
    }
    it->polys.push_back(o.poly[i]);
    it->values.push_back(i);
  }
  sort_points(o, less, &plan->super_points);
}

// False when two openings of one (polynomial, point) claim different values.
template <class Less>
bool group_by_poly_and_points(const Openings& o, Less less, Plan* plan) {
  plan->groups.clear();
  plan->super_points.clear();
  // per polynomial, in order of first appearance: its distinct points and
  // the opening that gives the value at each
  struct PolyPoints {
    size_t poly;
    std::vector<size_t> points, values;
  };
  std::vector<PolyPoints> by_poly;
  for (size_t i = 0; i < o.count; ++i) {
    const size_t pt = first_at_point(o, i);
    if (pt == i) plan->super_points.push_back(pt);
    auto it = std::find_if(by_poly.begin(), by_poly.end(), [&](const PolyPoints& p) { return p.poly == o.poly[i]; });
    if (it == by_poly.end()) {
      by_poly.push_back(PolyPoints{o.poly[i], {}, {}});
      it = by_poly.end() - 1;
    }
    const auto at = std::find(it->points.begin(), it->points.end(), pt);
    if (at == it->points.end()) {
      it->points.push_back(pt);
      it->values.push_back(i);
    } else if (!o.same_value(it->values[at - it->points.begin()], i)) {
      return false;
    }
  }
  sort_points(o, less, &plan->super_points);
  for (PolyPoints& p : by_poly) {
    // order the set (and the values with it)
    std::vector<size_t> order(p.points.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    std::sort(order.begin(), order.end(),
              [&](size_t a, size_t b) { return less(o.point(p.points[a]), o.point(p.points[b])); });
    std::vector<size_t> pts, vals;
    for (size_t k : order) pts.push_back(p.points[k]), vals.push_back(p.values[k]);
    auto it = std::find_if(plan->groups.begin(), plan->groups.end(), [&](const Group& g) { return g.points == pts; });
    if (it == plan->groups.end()) {
      plan->groups.push_back(Group{pts, {}, {}});
      it = plan->groups.end() - 1;
    }
    it->polys.push_back(p.poly);
    it->values.insert(it->values.end(), vals.begin(), vals.end());
  }
  return true;
}

// Validation and grouping together: false (plan untouched by the caller's
// standards: do not use it) on any refusal.
template <class Less>
bool make_plan(int scheme, const Openings& o, const size_t* lens, size_t num_polys, size_t n, Less less, Plan* plan) {
  if (!scheme_ok(scheme) || !arguments_ok(o, lens, num_polys, n)) return false;
  if (scheme == kGwc) {
    group_by_single_point(o, less, plan);
    return true;
  }
  return group_by_poly_and_points(o, less, plan);
}

// Words of the flat form of a plan: the group count, then per group the
// point count, the points (elem_bytes / 8 words each), the polynomial count
// and the polynomial indices.
inline size_t flat_words(const Plan& plan, size_t elem_bytes) {
  size_t w = 1;
  for (const Group& g : plan.groups) w += 2 + g.points.size() * (elem_bytes / 8) + g.polys.size();
  return w;
}

inline void flatten(const Plan& plan, const Openings& o, uint64_t* out) {
  *out++ = plan.groups.size();
  for (const Group& g : plan.groups) {
    *out++ = g.points.size();
    for (size_t pt : g.points) {
      memcpy(out, o.point(pt), o.elem_bytes);
      out += o.elem_bytes / 8;
    }
    *out++ = g.polys.size();
    for (size_t p : g.polys) *out++ = p;
  }
}

}  // namespace tachyon_amd::kzg_open
