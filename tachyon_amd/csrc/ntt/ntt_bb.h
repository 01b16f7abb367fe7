// BabyBear NTT on the GPU: the engine of IcicleNTT<BabyBear>
// (icicle_ntt_baby_bear.cc:31-115) and of Radix2EvaluationDomain::FFTBatch /
// CosetLDEBatch (radix2_evaluation_domain.h:99-197) on a row-major matrix.
//
// BbGenDomain is shaped like NttGenDomain: initialised from a generator g of
// order N = 2^LN (0 <= LN <= 27), it serves every size n = 2^L <= N with
// w_n = g^(N/n), on any coset, forward and inverse, natural order in and out.
// Elements are Montgomery words (field/bb31.h).
//
// Two layouts, one pass kernel.  A transform is a sequence of at most three
// Stockham passes of radix R = 2^k <= 2^10: with n_cur = R m the length of the
// sub-transforms still to do and s the number of them interleaved, a pass
// reads x[q + s (p + m j)], takes the R-point DFT over j in LDS, multiplies
// output k by w_(n_cur)^(p k) and writes y[q + s (k + R p)].  With C columns
// riding along as the fastest dimension (q' = q C + c, s' = s C) the pass is a
// tile of R rows (stride m s' words) by T adjacent words, lanes along the
// contiguous dimension:
//   consecutive: C = 1, `batch` arrays one after another
//   columns:     a rows x cols row-major matrix, C = cols, every column one
//                transform; no transpose through memory
// The first passes write out of place (data -> scratch -> data); the last pass
// of every plan has m = 1, reads and writes the same tile, and runs in place.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/hip_util.h"

namespace tachyon_amd::ntt {

class BbGenDomain {
 public:
  static constexpr uint32_t kMaxLogOrder = 27;   // BabyBear's two-adicity
  static constexpr uint32_t kMaxPassStages = 10; // R <= 2^10 rows per tile
  static constexpr size_t kCosetCacheEntries = 8;

  explicit BbGenDomain(hipStream_t stream = nullptr);
  ~BbGenDomain();
  BbGenDomain(const BbGenDomain&) = delete;
  BbGenDomain& operator=(const BbGenDomain&) = delete;

  // group_gen (Montgomery, < p) must have order exactly 2^LN, LN <= 27; false
  // otherwise, or when initialised with another generator (the same one: a
  // no-op).  Synchronises.
  bool init(uint32_t group_gen);
  bool initialised() const { return inited_; }
  int log_order() const { return inited_ ? (int)log_n_ : -1; }
  uint32_t group_gen() const { return gen_; }
  hipStream_t stream() const { return stream_; }
  size_t table_bytes() const;  // twiddle tables + cached power tables
  void release();

  // Stages per pass of a 2^log_m-point transform: one pass up to 2^10, two up
  // to 2^20, three up to 2^27.
  static std::vector<uint32_t> plan(uint32_t log_m);

  // In place on `batch` consecutive device arrays of 2^log_m words, on the
  // coset h<w_m> (Montgomery h; one = the plain sub-domain), enqueued on
  // stream().  batch * 2^log_m < 2^32.
  void run(uint32_t* d_data, uint32_t log_m, bool inverse, size_t batch, uint32_t coset);
  void run_host(uint32_t* data, uint32_t log_m, bool inverse, size_t batch, uint32_t coset);

  // In place on every column of a row-major 2^log_rows x cols device matrix.
  // cols >= 1, 2^log_rows * cols < 2^32.
  void run_columns(uint32_t* d_mat, uint32_t log_rows, size_t cols, bool inverse, uint32_t coset);
  void run_columns_host(uint32_t* mat, uint32_t log_rows, size_t cols, bool inverse, uint32_t coset);

  // CosetLDEBatch: per column, the inverse transform at 2^log_rows, coefficient
  // j times shift^j / rows, zero padding to rows << added_bits, the forward
  // transform at that size; natural order.  d_in is not written (d_in == d_out
  // is allowed: every pass that reads d_in is enqueued before the first that
  // writes d_out).  (2^log_rows << added_bits) * cols < 2^32.
  void coset_lde(const uint32_t* d_in, uint32_t log_rows, size_t cols, uint32_t added_bits, uint32_t shift,
                 uint32_t* d_out);
  void coset_lde_host(const uint32_t* in, uint32_t log_rows, size_t cols, uint32_t added_bits, uint32_t shift,
                      uint32_t* out);

  // kernel launches of the last run / run_columns / coset_lde
  unsigned last_launches() const { return launches_; }

 private:
  // two-level powers of one base b: lo[i] = b^i (i < 2^lb), hi[j] = b^(j 2^lb)
  struct Powers {
    uint32_t base = 0;
    uint64_t used = 0;  // 0: empty
    DeviceBuffer lo, hi;
  };
  void build_powers(Powers& t, uint32_t base);
  const Powers& powers(uint32_t base);
  // src -> dst through tmp, `batch` items of 2^log_n x cols words; rows >=
  // rows_valid of src (compact, batch 1) read as zero
  void transform(const uint32_t* src, uint32_t* dst, uint32_t* tmp, uint32_t log_n, uint32_t cols, uint32_t batch,
                 bool inverse, const Powers* load_cs, const Powers* store_cs, bool scale, uint32_t rows_valid);

  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;
  bool inited_ = false;
  uint32_t log_n_ = 0, lb_ = 0;
  uint32_t gen_ = 0;
  Powers fwd_, inv_;
  Powers cosets_[kCosetCacheEntries];
  uint64_t tick_ = 0;
  DeviceBuffer scratch_, lde_, io_, io2_;
  unsigned launches_ = 0;
};

}  // namespace tachyon_amd::ntt
