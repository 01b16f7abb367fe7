// What a C-ABI entry point does when its body throws (host-only, no HIP).
// Nothing unwinds across extern "C"; each entry point takes one of three
// policies, by the kind of function it is:
//   abort            GUARD_BEGIN .. GUARD_END: the reference-ABI functions and
//                    their extensions (MSM, domains, KZG, Groth16, dist) abort
//                    with a message, like the reference's CHECK
//                    (msm.h:42-43, msm_gpu.h:79-80).
//   silent fallback  guarded(): the drop-in Icicle and BabyBear entry points
//                    (icicle_ntt, merkle, fri) return false / 0 / nullptr.
//   report, return 0 guarded_report(): collective and batch entry points
//                    (sharded plan MSM, grand products) print the same message
//                    and return 0, so that every rank or the whole batch fails
//                    together.
// Early refusals (device-pointer checks, size mismatches, null handles) stay in
// front of the guard: they return before anything can throw.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <exception>

namespace tachyon_amd {

inline void report_failure(const char* fn, const char* what) {
  fprintf(stderr, "[tachyon_mi355x] %s failed: %s\n", fn, what);
  fflush(stderr);
}

[[noreturn]] inline void die(const char* fn, const char* what) {
  report_failure(fn, what);
  abort();
}

// What `body` returns, or `fallback` if it throws.  A bool becomes the entry
// point's 1 or 0.
template <class T, class Fn>
T guarded(T fallback, Fn&& body) {
  try {
    return body();
  } catch (...) {
    return fallback;
  }
}

// guarded() with the failure on stderr under the entry point's name (pass
// __func__: inside the lambda it would name operator()).
template <class T, class Fn>
T guarded_report(const char* fn, T fallback, Fn&& body) {
  try {
    return body();
  } catch (const std::exception& e) {
    report_failure(fn, e.what());
  } catch (...) {
    report_failure(fn, "unknown exception");
  }
  return fallback;
}

}  // namespace tachyon_amd

// Macros, not a lambda: a `return` in the body leaves the entry point, and
// __func__ names it.
#define GUARD_BEGIN try {
#define GUARD_END                                                             \
  }                                                                           \
  catch (const std::exception& e) { ::tachyon_amd::die(__func__, e.what()); } \
  catch (...) { ::tachyon_amd::die(__func__, "unknown exception"); }
