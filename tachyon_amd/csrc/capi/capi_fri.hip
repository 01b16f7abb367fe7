// C-ABI of BabyBear4 and the FRI opening (include/tachyon_mi355x.h) over
// fri::FriOpening: int results, nothing aborts across this boundary.  The shape
// and phase rules live in fri_validate.h.
#include "../../../include/tachyon_mi355x.h"

#include <memory>

#include "../common/hip_util.h"
#include "../fri/fri_bb.h"
#include "capi_handles.h"
#include "fri_validate.h"
#include "merkle_tree_validate.h"

using namespace tachyon_amd;
using fri::Fp4;

extern "C" {

int tachyon_mi355x_baby_bear4_ops(int op, const void* a, const void* b, void* out, size_t count, void* stream) {
  const bool binary = op == fri::kBb4Add || op == fri::kBb4Sub || op == fri::kBb4Mul;
  if (op < 0 || op >= fri::kBb4NumOps || !a || !out || (binary && !b) || count == 0 || count > (size_t(1) << 28))
    return 0;
  return guarded(0, [&] {
    require_gpu();
    if (!binary) b = a;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool dev = is_device_pointer(a);
    if (is_device_pointer(b) != dev || is_device_pointer(out) != dev) return 0;
    if (dev) {
      fri::bb4_ops(op, static_cast<const Fp4*>(a), static_cast<const Fp4*>(b), static_cast<Fp4*>(out), count, s);
      if (!s) TA_HIP(hipStreamSynchronize(s));
      return 1;
    }
    const size_t bytes = count * sizeof(Fp4);
    DeviceBuffer d;
    Fp4* da = static_cast<Fp4*>(d.ensure(2 * bytes));
    Fp4* db = da + count;
    TA_HIP(hipMemcpyAsync(da, a, bytes, hipMemcpyHostToDevice, s));
    TA_HIP(hipMemcpyAsync(db, b, bytes, hipMemcpyHostToDevice, s));
    fri::bb4_ops(op, da, db, da, count, s);
    TA_HIP(hipMemcpyAsync(out, da, bytes, hipMemcpyDeviceToHost, s));
    TA_HIP(hipStreamSynchronize(s));
    return 1;
  });
}

tachyon_mi355x_baby_bear_fri_opening* tachyon_mi355x_baby_bear_fri_opening_create(unsigned log_blowup,
                                                                                   int external_matrix, void* stream) {
  if (!fri::log_blowup_ok(log_blowup) || !merkle_tree::external_ok(external_matrix)) return nullptr;
  return guarded<tachyon_mi355x_baby_bear_fri_opening*>(nullptr, [&] {
    auto h = std::make_unique<tachyon_mi355x_baby_bear_fri_opening>();
    h->fri = std::make_unique<fri::FriOpening>(log_blowup, external_matrix, static_cast<hipStream_t>(stream));
    return h.release();
  });
}

void tachyon_mi355x_baby_bear_fri_opening_destroy(tachyon_mi355x_baby_bear_fri_opening* h) {
  try {
    delete h;
  } catch (...) {
  }
}

int tachyon_mi355x_baby_bear_fri_opening_begin(tachyon_mi355x_baby_bear_fri_opening* h, const void* alpha) {
  if (!h || !alpha) return 0;
  return guarded(0, [&] { return h->fri->begin(fri::load_ext(alpha, 0)); });
}

int tachyon_mi355x_baby_bear_fri_opening_add_round(tachyon_mi355x_baby_bear_fri_opening* h, const void* const* ldes,
                                                   const size_t* rows, const size_t* cols, size_t count,
                                                   const void* const* points, const size_t* num_points,
                                                   void* const* opened_values_out) {
  if (!h) return 0;
  return guarded(0, [&] { return h->fri->add_round(ldes, rows, cols, count, points, num_points, opened_values_out); });
}

size_t tachyon_mi355x_baby_bear_fri_opening_num_inputs(const tachyon_mi355x_baby_bear_fri_opening* h) {
  return h ? h->fri->num_inputs() : 0;
}

unsigned tachyon_mi355x_baby_bear_fri_opening_input_log_size(const tachyon_mi355x_baby_bear_fri_opening* h, size_t k) {
  return h ? h->fri->input_log_size(k) : 0;
}

int tachyon_mi355x_baby_bear_fri_opening_input(tachyon_mi355x_baby_bear_fri_opening* h, size_t k, void* out) {
  if (!h || !out) return 0;
  return guarded(0, [&] { return h->fri->input(k, out); });
}

const void* tachyon_mi355x_baby_bear_fri_opening_input_device_ptr(const tachyon_mi355x_baby_bear_fri_opening* h,
                                                                  size_t k) {
  return h ? h->fri->input_device(k) : nullptr;
}

int tachyon_mi355x_baby_bear_fri_opening_commit(tachyon_mi355x_baby_bear_fri_opening* h, void* root_out) {
  if (!h || !root_out) return 0;
  return guarded(0, [&] { return h->fri->commit(root_out) == 1; });
}

int tachyon_mi355x_baby_bear_fri_opening_fold(tachyon_mi355x_baby_bear_fri_opening* h, const void* beta) {
  if (!h || !beta) return 0;
  return guarded(0, [&] { return h->fri->fold(fri::load_ext(beta, 0)); });
}

size_t tachyon_mi355x_baby_bear_fri_opening_num_commits(const tachyon_mi355x_baby_bear_fri_opening* h) {
  return h ? h->fri->num_commits() : 0;
}

int tachyon_mi355x_baby_bear_fri_opening_final_poly(tachyon_mi355x_baby_bear_fri_opening* h, void* out) {
  if (!h || !out) return 0;
  return guarded(0, [&] { return h->fri->final_poly(out); });
}

int tachyon_mi355x_baby_bear_fri_opening_answer_query(tachyon_mi355x_baby_bear_fri_opening* h, size_t index,
                                                      void* sibling_values_out, void* siblings_out) {
  if (!h) return 0;
  return guarded(0, [&] { return h->fri->answer_query(index, sibling_values_out, siblings_out); });
}

unsigned tachyon_mi355x_baby_bear_fri_opening_last_launches(const tachyon_mi355x_baby_bear_fri_opening* h) {
  return h ? h->fri->last_launches() : 0;
}

void* tachyon_mi355x_baby_bear_fri_opening_stream(tachyon_mi355x_baby_bear_fri_opening* h) {
  return h ? static_cast<void*>(h->fri->stream()) : nullptr;
}

}  // extern "C"
