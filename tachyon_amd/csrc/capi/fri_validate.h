// Argument checks and the phase rules of the
// tachyon_mi355x_baby_bear_fri_opening_* entry points
// (include/tachyon_mi355x.h): host-only C++ with no HIP dependency, so the
// refusal rules can be compiled and run on their own.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../common/bits.h"

namespace tachyon_amd::fri {

inline constexpr unsigned kMaxLogRows = 27;               // BabyBear's two-adicity
inline constexpr unsigned kMaxLogBlowup = 26;             // a fold step needs a root of order 2 rows
inline constexpr size_t kMaxCols = size_t(1) << 24;       // the tree's limit on one row

using bits::bit_reverse;
using bits::is_pow2;

// log2 of a power of two
inline unsigned log2_exact(size_t n) { return bits::ceil_log2(n); }

inline bool log_blowup_ok(unsigned log_blowup) { return log_blowup >= 1 && log_blowup <= kMaxLogBlowup; }

// an extension of `rows` x `cols` words: rows a power of two in
// [2^log_blowup, 2^27], at least one column (the reference underflows on none)
inline bool matrix_ok(size_t rows, size_t cols, unsigned log_blowup) {
  return log_blowup_ok(log_blowup) && cols != 0 && cols <= kMaxCols && is_pow2(rows) &&
         rows >= (size_t(1) << log_blowup) && rows <= (size_t(1) << kMaxLogRows);
}

// add_round's arguments.  points[m] and opened_values_out[m] may be null only
// for a matrix without points.
inline bool round_ok(const void* const* ldes, const size_t* rows, const size_t* cols, size_t count,
                     const void* const* points, const size_t* num_points, void* const* opened_values_out,
                     unsigned log_blowup) {
  if (!ldes || !rows || !cols || !points || !num_points || !opened_values_out || count == 0) return false;
  for (size_t m = 0; m < count; ++m) {
    if (!ldes[m] || !matrix_ok(rows[m], cols[m], log_blowup)) return false;
    if (num_points[m] != 0 && (!points[m] || !opened_values_out[m])) return false;
  }
  return true;
}

// Where a handle stands between begin() and the last answer_query().
struct Phase {
  bool begun = false;     // begin() has set alpha
  bool poisoned = false;  // a zero denominator was found on the device: only begin() helps
  bool started = false;   // the first commit() has frozen the inputs
  bool pending = false;   // commit() handed out a root that fold() has not consumed
  unsigned log_blowup = 0;
  unsigned log_max = 0;   // log2 of the largest input (valid once an input exists)
  bool has_input = false;
  unsigned log_size = 0;  // log2 of the current folded vector (valid once started)
};

inline bool usable(const Phase& p) { return p.begun && !p.poisoned; }
inline bool can_add_round(const Phase& p) { return usable(p) && !p.started; }
inline bool can_commit(const Phase& p) { return usable(p) && p.has_input && !p.pending; }
// whether a commit() now builds a tree (true) or reports the phase's end (false)
inline bool commit_has_work(const Phase& p) { return (p.started ? p.log_size : p.log_max) > p.log_blowup; }
inline bool can_fold(const Phase& p) { return usable(p) && p.started && p.pending; }
inline bool ended(const Phase& p) { return usable(p) && p.started && !p.pending && p.log_size <= p.log_blowup; }
inline bool can_answer(const Phase& p, size_t index) { return ended(p) && index < (size_t(1) << p.log_max); }

// commit-phase tree i of a query: the leaf (pair) index, the sibling's element
// in the folded vector, and the number of sibling digests
inline size_t query_pair(size_t index, unsigned i) { return (index >> i) >> 1; }
inline size_t query_sibling_element(size_t index, unsigned i) { return (index >> i) ^ 1; }
inline unsigned query_num_siblings(unsigned log_max, unsigned i) { return log_max - i - 1; }
// digests of all commit-phase openings of one query
inline size_t query_total_siblings(unsigned log_max, unsigned num_commits) {
  size_t total = 0;
  for (unsigned i = 0; i < num_commits; ++i) total += query_num_siblings(log_max, i);
  return total;
}

}  // namespace tachyon_amd::fri
