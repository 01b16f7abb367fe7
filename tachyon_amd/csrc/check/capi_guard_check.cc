// Host-only check of capi/capi_guard.h (no library, no HIP): guarded() and
// guarded_report() return the body's value or the fallback, the report is the
// exact "[tachyon_mi355x] <name> failed: <what>" line on stderr, and a
// GUARD_BEGIN .. GUARD_END body that does not throw returns its value.  The
// abort path is not exercised.  Not part of `all`:
//   make ../bin/capi_guard_check [CXX=... HOST_CHECK_FLAGS=-fsanitize=address,undefined]
#include <unistd.h>

#include <cstdio>
#include <stdexcept>
#include <string>

#include "../capi/capi_guard.h"

namespace {

using tachyon_amd::guarded;
using tachyon_amd::guarded_report;

int failures = 0;
void expect(bool ok, const char* what) {
  if (ok) return;
  printf("FAIL: %s\n", what);
  ++failures;
}

// what fn() writes to stderr, through a temporary file
template <class Fn>
std::string stderr_of(Fn&& fn) {
  fflush(stderr);
  FILE* tmp = tmpfile();
  if (!tmp) return "<no temporary file>";
  const int saved = dup(fileno(stderr));
  dup2(fileno(tmp), fileno(stderr));
  fn();
  fflush(stderr);
  dup2(saved, fileno(stderr));
  close(saved);
  rewind(tmp);
  std::string text;
  char buf[256];
  for (size_t got; (got = fread(buf, 1, sizeof(buf), tmp)) > 0;) text.append(buf, got);
  fclose(tmp);
  return text;
}

int entry_point_returning(int v) {
  GUARD_BEGIN
  if (v < 0) throw std::runtime_error("never taken here");
  return v;
  GUARD_END
}

void entry_point_void(int* out) {
  GUARD_BEGIN *out = 7; GUARD_END
}

}  // namespace

int main() {
  // guarded: the value, or the fallback on any throw, with nothing on stderr
  const std::string quiet = stderr_of([] {
    expect(guarded(0, [] { return 5; }) == 5, "guarded returns the body's value");
    expect(guarded(0, [] { return true; }) == 1, "guarded turns a bool into 1");
    expect(guarded(-1, []() -> int { throw std::runtime_error("x"); }) == -1, "guarded: std::exception -> fallback");
    expect(guarded(-2, []() -> int { throw 42; }) == -2, "guarded: non-std throw -> fallback");
    int dummy = 0;
    expect(guarded<int*>(nullptr, [&]() -> int* { throw std::string("s"); }) == nullptr, "guarded: pointer fallback");
    expect(guarded<int*>(nullptr, [&] { return &dummy; }) == &dummy, "guarded: pointer value");
  });
  expect(quiet.empty(), "guarded writes nothing to stderr");

  // guarded_report: the same, and the one line under the name it was given
  int got = -9;
  std::string text = stderr_of([&] { got = guarded_report("entry_a", 0, [] { return 1; }); });
  expect(got == 1 && text.empty(), "guarded_report returns the body's value and stays quiet");
  text = stderr_of([&] {
    got = guarded_report("entry_b", 0, []() -> int { throw std::runtime_error("null communicator"); });
  });
  expect(got == 0, "guarded_report: std::exception -> fallback");
  expect(text == "[tachyon_mi355x] entry_b failed: null communicator\n", "guarded_report: the std::exception line");
  text = stderr_of([&] { got = guarded_report("entry_c", -3, []() -> int { throw 42; }); });
  expect(got == -3, "guarded_report: non-std throw -> fallback");
  expect(text == "[tachyon_mi355x] entry_c failed: unknown exception\n", "guarded_report: the unknown exception line");

  // the aborting guard around bodies that do not throw
  expect(entry_point_returning(11) == 11, "GUARD_BEGIN .. GUARD_END returns the body's value");
  int v = 0;
  entry_point_void(&v);
  expect(v == 7, "GUARD_BEGIN .. GUARD_END runs a void body");

  if (failures == 0) printf("capi_guard_check ok\n");
  return failures ? 1 : 0;
}
