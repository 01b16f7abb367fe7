// C-ABI of the MI355X backend (include/tachyon_mi355x.h): version, device
// count and the generator and element-wise ops the tests and benchmarks use.
// Every subsystem has its own capi_<subsystem>.hip; capi_guard.h says what an
// entry point does when its body throws.
#include "../../../include/tachyon_mi355x.h"

#include "../util/device_ops.h"
#include "capi_guard.h"

using namespace tachyon_amd;

extern "C" {

const char* tachyon_mi355x_version(void) { return "tachyon_mi355x 0.1 (gfx950)"; }
int tachyon_mi355x_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void tachyon_mi355x_gen_scalars(int field, uint64_t seed, size_t start, size_t n, void* d_out, void* stream) {
  GUARD_BEGIN util::gen_scalars(field, seed, start, n, d_out, static_cast<hipStream_t>(stream)); GUARD_END
}
void tachyon_mi355x_gen_bases(int curve, uint64_t seed, size_t n, size_t chunk, void* d_out, void* stream) {
  GUARD_BEGIN util::gen_bases(curve, seed, 0, n, chunk, d_out, static_cast<hipStream_t>(stream)); GUARD_END
}
void tachyon_mi355x_gen_bases_at(int curve, uint64_t seed, size_t start, size_t n, size_t chunk, void* d_out,
                                 void* stream) {
  GUARD_BEGIN util::gen_bases(curve, seed, start, n, chunk, d_out, static_cast<hipStream_t>(stream)); GUARD_END
}
void tachyon_mi355x_field_op(int field, int op, const void* a, const void* b, void* out, size_t count) {
  GUARD_BEGIN util::field_op(field, op, a, b, out, count); GUARD_END
}
void tachyon_mi355x_ec_op(int curve, int op, const void* a, const void* b, void* out, size_t count) {
  GUARD_BEGIN util::ec_op(curve, op, a, b, out, count); GUARD_END
}
void tachyon_mi355x_limb_op(int family, int op, const uint32_t* in, uint32_t* out, size_t count) {
  GUARD_BEGIN util::limb_op(family, op, in, out, count); GUARD_END
}
int tachyon_mi355x_limb_op_words(int family, int op, int* in_words, int* out_words) {
  return util::limb_op_words(family, op, in_words, out_words) ? 1 : 0;
}

}  // extern "C"
