// C-ABI of the field-generic NTT domains and of the drop-in IcicleNTT engine
// with its BabyBear path (include/tachyon_mi355x.h).
#include "../../../include/tachyon_mi355x.h"

#include <cstring>
#include <memory>
#include <string>
#include <type_traits>

#include "../ntt/ntt.h"
#include "../ntt/ntt_bb.h"
#include "../field/bb31.h"  // (after the HIP runtime that ntt.h brings)
#include "capi_guard.h"
#include "icicle_ntt_validate.h"

using namespace tachyon_amd;

// ---- field-generic NTT domains ----
// Radix2EvaluationDomain<F> on the GPU for bn254 Fr (field 1) and bls12_381
// Fr (field 3): the engine of the IcicleNTT<F> holder
// (icicle_ntt_bls12_381.cc:31-115 for BLS12-381).
struct tachyon_mi355x_ntt_domain {
  int field = 0;
  std::unique_ptr<ntt::NttDomain<Bn254Fr>> bn;
  std::unique_ptr<ntt::NttDomain<Bls381Fr>> bls;
};

namespace {
template <class Fn>
void ntt_dispatch(const tachyon_mi355x_ntt_domain* d, Fn&& fn) {
  if (d->bn) fn(*d->bn);
  else fn(*d->bls);
}
}  // namespace

extern "C" {

tachyon_mi355x_ntt_domain* tachyon_mi355x_ntt_domain_create(int field, size_t num_coeffs) {
  if (field != 1 && field != 3) return nullptr;
  GUARD_BEGIN
  auto d = std::make_unique<tachyon_mi355x_ntt_domain>();
  d->field = field;
  if (field == 1) d->bn = std::make_unique<ntt::NttDomain<Bn254Fr>>(num_coeffs);
  else d->bls = std::make_unique<ntt::NttDomain<Bls381Fr>>(num_coeffs);
  return d.release();
  GUARD_END
  return nullptr;
}
void tachyon_mi355x_ntt_domain_destroy(tachyon_mi355x_ntt_domain* d) { delete d; }
size_t tachyon_mi355x_ntt_domain_size(const tachyon_mi355x_ntt_domain* d) {
  size_t n = 0;
  ntt_dispatch(d, [&](auto& dom) { n = dom.size(); });
  return n;
}
int tachyon_mi355x_ntt_domain_field(const tachyon_mi355x_ntt_domain* d) { return d->field; }
void tachyon_mi355x_ntt_domain_group_gen(const tachyon_mi355x_ntt_domain* d, void* out) {
  ntt_dispatch(d, [&](auto& dom) { memcpy(out, &dom.group_gen(), sizeof(dom.group_gen())); });
}
void tachyon_mi355x_ntt_domain_set_offset(tachyon_mi355x_ntt_domain* d, const void* offset) {
  GUARD_BEGIN
  ntt_dispatch(d, [&](auto& dom) {
    using Fr = std::decay_t<decltype(dom.group_gen())>;
    Fr h = Fr::one();
    if (offset) memcpy(&h, offset, sizeof(h));
    dom.set_offset(h);
  });
  GUARD_END
}
void tachyon_mi355x_ntt_domain_transform_host(tachyon_mi355x_ntt_domain* d, void* inout, size_t len, int inverse) {
  GUARD_BEGIN
  ntt_dispatch(d, [&](auto& dom) {
    using Fr = std::decay_t<decltype(dom.group_gen())>;
    if (len != dom.size())
      throw std::runtime_error("transform_host: the vector must hold exactly size() elements (" +
                               std::to_string(len) + " != " + std::to_string(dom.size()) + ")");
    auto* v = static_cast<Fr*>(inout);
    if (inverse) dom.inverse_host(v, len, v);
    else dom.forward_host(v, len, v);
  });
  GUARD_END
}
void tachyon_mi355x_ntt_domain_transform_device(tachyon_mi355x_ntt_domain* d, void* d_data, size_t batch,
                                                int inverse) {
  GUARD_BEGIN
  ntt_dispatch(d, [&](auto& dom) {
    using Fr = std::decay_t<decltype(dom.group_gen())>;
    auto* x = static_cast<Fr*>(d_data);
    if (inverse) dom.inverse_device(x, batch);
    else dom.forward_device(x, batch);
  });
  GUARD_END
}
void* tachyon_mi355x_ntt_domain_stream(tachyon_mi355x_ntt_domain* d) {
  void* s = nullptr;
  ntt_dispatch(d, [&](auto& dom) { s = static_cast<void*>(dom.stream()); });
  return s;
}

}  // extern "C"

// ---- the drop-in IcicleNTT engine ----
// IcicleNTT<F>::Init / Run / Release (icicle_ntt.h:43-87,
// icicle_ntt_bn254.cc:31-116) over ntt::NttGenDomain: bool results, nothing
// aborts across this boundary (guarded(), capi_guard.h).
struct tachyon_mi355x_icicle_ntt {
  int field = 0;
  std::unique_ptr<ntt::NttGenDomain<Bn254Fr>> bn;
  std::unique_ptr<ntt::NttGenDomain<Bls381Fr>> bls;
  std::unique_ptr<ntt::BbGenDomain> bb;  // field 4: 4-byte elements, its own entry paths below
  tachyon_mi355x_icicle_ntt_options options = icicle_ntt::default_options();
};

namespace {
template <class Fn>
void icicle_ntt_dispatch(const tachyon_mi355x_icicle_ntt* h, Fn&& fn) {
  if (h->bn) fn(*h->bn);
  else fn(*h->bls);
}

// ---- baby_bear (field 4) over ntt::BbGenDomain ----
int bb_init(tachyon_mi355x_icicle_ntt* h, const void* group_gen_mont, const tachyon_mi355x_icicle_ntt_options& opt) {
  if (!icicle_ntt::options_ok_columns(opt)) return 0;
  uint32_t g;
  memcpy(&g, group_gen_mont, sizeof(g));
  if (g >= bb31::kP) return 0;  // not a Montgomery representative
  const bool fresh = !h->bb->initialised();
  if (!h->bb->init(g)) return 0;
  if (fresh) h->options = opt;
  return 1;
}

// rows x cols words with both counts checked against the 32-bit indexing of the passes
bool bb_fits(size_t rows, size_t cols) { return cols != 0 && cols < (uint64_t(1) << 32) / rows; }

// consecutive (cols == 0: `batch` arrays of `size`) or columns (a size x cols matrix)
int bb_run(tachyon_mi355x_icicle_ntt* h, const void* coset_canonical, void* inout, size_t size, size_t batch,
           size_t cols, int inverse) {
  ntt::BbGenDomain& dom = *h->bb;
  const int log_m = icicle_ntt::size_log(size, dom.log_order());
  if (log_m < 0) return 0;
  uint32_t c;
  if (!icicle_ntt::small_coset(coset_canonical, bb31::kP, &c)) return 0;
  if (!bb_fits(size, cols ? cols : batch)) return 0;
  const uint32_t coset = bb31::to_mont(c);
  const tachyon_mi355x_icicle_ntt_options& o = h->options;
  auto* x = static_cast<uint32_t*>(inout);
  if (o.are_inputs_on_device) {
    if (cols) dom.run_columns(x, (uint32_t)log_m, cols, inverse != 0, coset);
    else dom.run(x, (uint32_t)log_m, inverse != 0, batch, coset);
    if (!o.is_async) TA_HIP(hipStreamSynchronize(dom.stream()));
  } else {
    if (cols) dom.run_columns_host(x, (uint32_t)log_m, cols, inverse != 0, coset);
    else dom.run_host(x, (uint32_t)log_m, inverse != 0, batch, coset);
  }
  return 1;
}
}  // namespace

extern "C" {

tachyon_mi355x_icicle_ntt* tachyon_mi355x_icicle_ntt_create(int field, void* stream) {
  if (field != 1 && field != 3 && field != 4) return nullptr;
  return guarded<tachyon_mi355x_icicle_ntt*>(nullptr, [&] {
    auto h = std::make_unique<tachyon_mi355x_icicle_ntt>();
    h->field = field;
    if (field == 4) h->bb = std::make_unique<ntt::BbGenDomain>(static_cast<hipStream_t>(stream));
    else if (field == 1) h->bn = std::make_unique<ntt::NttGenDomain<Bn254Fr>>(static_cast<hipStream_t>(stream));
    else h->bls = std::make_unique<ntt::NttGenDomain<Bls381Fr>>(static_cast<hipStream_t>(stream));
    return h.release();
  });
}

int tachyon_mi355x_icicle_ntt_init(tachyon_mi355x_icicle_ntt* h, const void* group_gen_mont,
                                   const tachyon_mi355x_icicle_ntt_options* options) {
  if (!h || !group_gen_mont) return 0;
  const tachyon_mi355x_icicle_ntt_options opt = options ? *options : icicle_ntt::default_options();
  if (h->bb) return guarded(0, [&] { return bb_init(h, group_gen_mont, opt); });
  if (!icicle_ntt::options_ok(opt)) return 0;
  return guarded(0, [&] {
    int ok = 0;
    bool fresh = false;
    icicle_ntt_dispatch(h, [&](auto& dom) {
      using Fr = std::decay_t<decltype(dom.group_gen())>;
      uint32_t w[8];
      icicle_ntt::load_words(group_gen_mont, w);
      if (!icicle_ntt::below(w, Fr::Config::kP32)) return;  // not a Montgomery representative
      Fr g;
      for (int i = 0; i < 8; ++i) g.v[i] = w[i];
      fresh = !dom.initialised();
      ok = dom.init(g) ? 1 : 0;
    });
    if (ok && fresh) h->options = opt;  // (the same generator again: nothing changes)
    return ok;
  });
}

int tachyon_mi355x_icicle_ntt_run(tachyon_mi355x_icicle_ntt* h, int algorithm, const void* coset_canonical,
                                  void* inout, size_t size, int inverse) {
  (void)algorithm;  // Auto / Radix2 / MixedRadix: one network, one result
  if (!h || !coset_canonical || !inout) return 0;
  if (h->bb)
    return guarded(0, [&] {
      const size_t batch = (size_t)h->options.batch_size;
      return h->options.columns_batch ? bb_run(h, coset_canonical, inout, size, 1, batch, inverse)
                                      : bb_run(h, coset_canonical, inout, size, batch, 0, inverse);
    });
  return guarded(0, [&] {
    int ok = 0;
    icicle_ntt_dispatch(h, [&](auto& dom) {
      using Fr = std::decay_t<decltype(dom.group_gen())>;
      const int log_m = icicle_ntt::size_log(size, dom.log_order());
      if (log_m < 0) return;
      uint32_t w[8];
      icicle_ntt::load_words(coset_canonical, w);
      if (!icicle_ntt::coset_ok(w, Fr::Config::kP32)) return;
      Fr c;
      for (int i = 0; i < 8; ++i) c.v[i] = w[i];
      const Fr coset = c.to_mont().canonical();
      const tachyon_mi355x_icicle_ntt_options& o = h->options;
      const size_t batch = (size_t)o.batch_size;
      if (batch > 65535) return;
      auto* x = static_cast<Fr*>(inout);
      if (o.are_inputs_on_device) {
        dom.run(x, (uint32_t)log_m, inverse != 0, batch, coset);
        if (!o.is_async) TA_HIP(hipStreamSynchronize(dom.stream()));
      } else {
        dom.run_host(x, (uint32_t)log_m, inverse != 0, batch, coset);
      }
      ok = 1;
    });
    return ok;
  });
}

int tachyon_mi355x_icicle_ntt_release(tachyon_mi355x_icicle_ntt* h) {
  if (!h) return 0;
  return guarded(0, [&] {
    if (h->bb) h->bb->release();
    else icicle_ntt_dispatch(h, [&](auto& dom) { dom.release(); });
    return 1;
  });
}

void tachyon_mi355x_icicle_ntt_destroy(tachyon_mi355x_icicle_ntt* h) {
  guarded(0, [&] {
    delete h;
    return 0;
  });
}

int tachyon_mi355x_icicle_ntt_log_order(const tachyon_mi355x_icicle_ntt* h) {
  int l = -1;
  if (h && h->bb) return h->bb->log_order();
  if (h) icicle_ntt_dispatch(h, [&](auto& dom) { l = dom.log_order(); });
  return l;
}

void* tachyon_mi355x_icicle_ntt_stream(tachyon_mi355x_icicle_ntt* h) {
  void* s = nullptr;
  if (h && h->bb) return static_cast<void*>(h->bb->stream());
  if (h) icicle_ntt_dispatch(h, [&](auto& dom) { s = static_cast<void*>(dom.stream()); });
  return s;
}

size_t tachyon_mi355x_icicle_ntt_table_bytes(const tachyon_mi355x_icicle_ntt* h) {
  size_t b = 0;
  if (h && h->bb) return h->bb->table_bytes();
  if (h) icicle_ntt_dispatch(h, [&](auto& dom) { b = dom.table_bytes(); });
  return b;
}

int tachyon_mi355x_icicle_ntt_run_matrix(tachyon_mi355x_icicle_ntt* h, int algorithm, const void* coset_canonical,
                                         void* inout, size_t rows, size_t cols, int inverse) {
  (void)algorithm;
  if (!h || !h->bb || !coset_canonical || !inout || cols == 0) return 0;
  return guarded(0, [&] { return bb_run(h, coset_canonical, inout, rows, 1, cols, inverse); });
}

int tachyon_mi355x_icicle_ntt_coset_lde_batch(tachyon_mi355x_icicle_ntt* h, const void* in, size_t rows, size_t cols,
                                              size_t added_bits, const void* shift_canonical, void* out) {
  if (!h || !h->bb || !in || !out || !shift_canonical || cols == 0) return 0;
  return guarded(0, [&] {
    ntt::BbGenDomain& dom = *h->bb;
    const int log_rows = icicle_ntt::size_log(rows, dom.log_order());
    if (log_rows < 0 || added_bits > (size_t)(dom.log_order() - log_rows)) return 0;
    if (in == out && added_bits > 0) return 0;
    uint32_t c;
    if (!icicle_ntt::small_coset(shift_canonical, bb31::kP, &c)) return 0;
    if (!bb_fits(rows << added_bits, cols)) return 0;
    const uint32_t shift = bb31::to_mont(c);
    const tachyon_mi355x_icicle_ntt_options& o = h->options;
    if (o.are_inputs_on_device) {
      dom.coset_lde(static_cast<const uint32_t*>(in), (uint32_t)log_rows, cols, (uint32_t)added_bits, shift,
                    static_cast<uint32_t*>(out));
      if (!o.is_async) TA_HIP(hipStreamSynchronize(dom.stream()));
    } else {
      dom.coset_lde_host(static_cast<const uint32_t*>(in), (uint32_t)log_rows, cols, (uint32_t)added_bits, shift,
                         static_cast<uint32_t*>(out));
    }
    return 1;
  });
}

unsigned tachyon_mi355x_icicle_ntt_last_launches(const tachyon_mi355x_icicle_ntt* h) {
  return h && h->bb ? h->bb->last_launches() : 0;
}

}  // extern "C"
