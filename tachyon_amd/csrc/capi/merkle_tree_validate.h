// Argument checks and the layer plan of the tachyon_mi355x_baby_bear_merkle_tree_*
// entry points (include/tachyon_mi355x.h): host-only C++ with no HIP
// dependency, so the refusal rules can be compiled and run on their own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/bits.h"

namespace tachyon_amd::merkle_tree {

inline constexpr unsigned kFlagBitReversed = 1u;  // TACHYON_MI355X_MERKLE_BIT_REVERSED
inline constexpr unsigned kKnownFlags = kFlagBitReversed;
inline constexpr size_t kMaxGroup = 16;                 // matrices hashed into one layer
inline constexpr size_t kMaxRows = size_t(1) << 30;     // leaves of the tallest matrix
inline constexpr size_t kMaxRowWords = size_t(1) << 24; // words of one concatenated row

// external_matrix ids: 0 Horizen, 1 Plonky3
inline bool external_ok(int id) { return id == 0 || id == 1; }

using bits::bit_ceil;
using bits::bit_reverse;
using bits::ceil_log2;
using bits::is_pow2;

// One digest layer: the matrices order[first .. first + count) are hashed into
// it (count == 0: plain compression), `rows` their common height.
struct Level {
  size_t size = 0;  // digests in the layer, a power of two
  size_t first = 0, count = 0, rows = 0;
};

struct Plan {
  std::vector<size_t> order;  // matrix ids, stable-sorted by height, descending
  std::vector<Level> levels;  // levels[0] the leaf layer .. levels.back() the root
  unsigned log_max = 0;
};

// FieldMerkleTree::Build's shape rules.  False for: null arrays, count 0, a
// matrix with 0 rows or columns, unknown flag bits, heights that round up to
// the same power of two but differ, the bit-reversed flag with a height that
// is not a power of two, and sizes beyond the limits above.
inline bool make_plan(const size_t* rows, const size_t* cols, size_t count, unsigned flags, Plan* plan) {
  if (!rows || !cols || !plan || count == 0 || (flags & ~kKnownFlags) != 0) return false;
  for (size_t i = 0; i < count; ++i) {
    if (rows[i] == 0 || cols[i] == 0 || rows[i] > kMaxRows || cols[i] > kMaxRowWords) return false;
    if ((flags & kFlagBitReversed) && !is_pow2(rows[i])) return false;
  }
  Plan p;
  p.order.resize(count);
  for (size_t i = 0; i < count; ++i) p.order[i] = i;
  std::stable_sort(p.order.begin(), p.order.end(), [&](size_t a, size_t b) { return rows[a] > rows[b]; });
  for (size_t i = 0; i + 1 < count; ++i) {
    const size_t a = rows[p.order[i]], b = rows[p.order[i + 1]];
    if (a != b && bit_ceil(a) == bit_ceil(b)) return false;
  }
  p.log_max = ceil_log2(rows[p.order[0]]);
  size_t at = 0;
  for (unsigned k = 0; k <= p.log_max; ++k) {
    Level l;
    l.size = size_t(1) << (p.log_max - k);
    l.first = at;
    size_t words = 0;
    while (at < count && bit_ceil(rows[p.order[at]]) == l.size) {
      words += cols[p.order[at]];
      ++at;
    }
    l.count = at - l.first;
    if (l.count > kMaxGroup || words > kMaxRowWords) return false;
    if (l.count) l.rows = rows[p.order[l.first]];
    p.levels.push_back(l);
  }
  if (at != count) return false;  // (unreachable: every height's bit_ceil is a level size)
  *plan = std::move(p);
  return true;
}

// digests before layer k in the layer buffer: size_0 + .. + size_(k-1)
inline size_t layer_offset(const Plan& p, size_t k) {
  size_t off = 0;
  for (size_t j = 0; j < k && j < p.levels.size(); ++j) off += p.levels[j].size;
  return off;
}

// DoCreateOpeningProof's row of a matrix with `rows` rows for leaf `index`:
// index >> (log_max - ceil_log2(rows)), bit-reversed over log2(rows) bits with
// the flag.  False when that row is past the matrix's height (the padded part
// of a height that is no power of two).
inline bool open_row(size_t index, unsigned log_max, size_t rows, unsigned flags, size_t* row) {
  const unsigned lg = ceil_log2(rows);
  size_t r = index >> (log_max - lg);
  if (flags & kFlagBitReversed) r = bit_reverse(r, lg);
  *row = r;
  return r < rows;
}

}  // namespace tachyon_amd::merkle_tree
