"""The grouping and validation behind the KZG opening entry points
(tachyon_amd/csrc/capi/kzg_open_validate.h, tachyon_mi355x_kzg_opening_plan):
host code, so it runs without a GPU.  The library's plan equals the
reference's grouping (tests/kzg_open_ref.py), every refusal returns None, the
header compiles on its own with a plain host compiler, and a small program
with its own main groups the fixture's pattern under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import kzg_open_ref as R
from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bn254_kzg_polynomial_openings.json")
HEADER_DIR = os.path.join(ROOT, "tachyon_amd", "csrc", "capi")
LIB = os.path.join(ROOT, "tachyon_amd", "libtachyon_mi355x.so")
Fr = pyref.Field("bn254_fr")


def lib_plan(scheme, lens, n, openings, curve="bn254_g1", field=Fr):
    from tachyon_amd.kzg import opening_plan
    got = opening_plan(curve, scheme, lens, n, [(i, field.to_bytes(x), field.to_bytes(v)) for i, x, v in openings])
    return None if got is None else [([field.from_bytes(p) for p in pts], polys) for pts, polys in got]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        pytest.fail("libtachyon_mi355x.so not built (run __graft_entry__.build())")


@pytest.fixture(scope="module")
def readings():
    polys, openings, _ = R.load_fixture(GOLDEN)
    merged, mo = R.merge_equal(polys, openings)
    return {"by_index": ([len(p) for p in polys], openings), "merged": ([len(p) for p in merged], mo)}


@pytest.mark.parametrize("scheme", [R.GWC, R.SHPLONK])
@pytest.mark.parametrize("reading", ["by_index", "merged"])
def test_plan_equals_reference_on_fixture(built, readings, scheme, reading):
    lens, openings = readings[reading]
    want = R.plan(scheme, lens, 16, openings)
    assert want is not None and lib_plan(scheme, lens, 16, openings) == want


def test_plan_small_cases(built):
    r = Fr.p
    cases = {
        "duplicate": [(0, 5, 7), (1, 5, 8), (0, 5, 7)],
        "one_poly_many_points": [(0, r - 1, 1), (0, 3, 2), (0, 0, 3), (1, 3, 4), (0, 3, 2)],
        "sets_in_any_order": [(0, 9, 1), (1, 4, 2), (0, 4, 3), (1, 9, 4), (2, 9, 5)],
        "empty": [],
    }
    for name, openings in cases.items():
        for scheme in (R.GWC, R.SHPLONK):
            want = R.plan(scheme, [4, 0, 2], 4, openings)
            assert want is not None and lib_plan(scheme, [4, 0, 2], 4, openings) == want, (name, scheme)
    # GWC keeps the duplicate, SHPlonk's point sets drop it
    assert lib_plan(R.GWC, [4, 0, 2], 4, cases["duplicate"]) == [([5], [0, 1, 0])]
    assert lib_plan(R.SHPLONK, [4, 0, 2], 4, cases["duplicate"]) == [([5], [0, 1])]
    # a group's points are in the field's order, not the order of appearance
    assert lib_plan(R.SHPLONK, [4, 0, 2], 4, cases["one_poly_many_points"]) == [([0, 3, r - 1], [0]), ([3], [1])]
    # the other scalar field
    bls = pyref.Field("bls12_381_fr")
    o = [(0, bls.p - 2, 1), (1, 6, 2), (0, 6, 3)]
    assert lib_plan(R.SHPLONK, [1, 1], 1, o, "bls12_381_g1", bls) == R.plan(R.SHPLONK, [1, 1], 1, o)


def test_refusals(built):
    import ctypes
    from tachyon_amd._lib import lib
    ok = [(0, 5, 7), (1, 6, 8)]
    for scheme in (R.GWC, R.SHPLONK):
        assert lib_plan(scheme, [4, 4], 4, ok) is not None
        assert lib_plan(scheme, [4, 4], 4, ok + [(2, 5, 7)]) is None  # index out of range
        assert lib_plan(scheme, [4, 4], 4, ok + [(-1, 5, 7)]) is None
        assert lib_plan(scheme, [4, 5], 4, ok) is None  # longer than N
    # the same (polynomial, point) with two values: SHPlonk only
    clash = ok + [(0, 5, 9)]
    assert lib_plan(R.SHPLONK, [4, 4], 4, clash) is None and R.plan(R.SHPLONK, [4, 4], 4, clash) is None
    assert lib_plan(R.GWC, [4, 4], 4, clash) == [([5], [0, 0]), ([6], [1])]
    # null arrays with a nonzero count, an unknown scheme or curve, too little room
    L = lib()
    lens = (ctypes.c_size_t * 2)(4, 4)
    idx = (ctypes.c_size_t * 2)(0, 1)
    pts = ctypes.create_string_buffer(Fr.to_bytes(5) + Fr.to_bytes(6), 64)
    out = (ctypes.c_uint64 * 32)()
    words = ctypes.c_size_t(0)
    args = lambda **kw: [kw.get("curve", 0), kw.get("scheme", 1), kw.get("lens", lens), 2, 4, kw.get("idx", idx),
                         kw.get("pts", pts), kw.get("vals", pts), 2, kw.get("out", out), kw.get("cap", 32),
                         ctypes.byref(words)]
    assert L.tachyon_mi355x_kzg_opening_plan(*args()) == 1 and words.value == 1 + 2 * (2 + 4 + 1)
    for bad in ({"lens": None}, {"idx": None}, {"pts": None}, {"vals": None}, {"scheme": 2}, {"curve": 1}, {"cap": 3},
                {"out": None}):
        assert L.tachyon_mi355x_kzg_opening_plan(*args(**bad)) == 0, bad


def test_header_compiles_alone(tmp_path):
    src = tmp_path / "use.cc"
    src.write_text('#include "kzg_open_validate.h"\n'
                   "bool f(const tachyon_amd::kzg_open::Openings& o, const size_t* lens, tachyon_amd::kzg_open::Plan* p) {\n"
                   "  auto less = [](const unsigned char* a, const unsigned char* b) { return a[0] < b[0]; };\n"
                   "  return tachyon_amd::kzg_open::make_plan(1, o, lens, 2, 16, less, p);\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", HEADER_DIR, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


MAIN = r"""
#include <cstdio>
#include <cstring>
#include "kzg_open_validate.h"
using namespace tachyon_amd::kzg_open;
// stdin: scheme, polynomial count, n, opening count, then per opening
// "poly point value" (small integers; 32-byte little-endian elements)
int main() {
  unsigned long scheme, num_polys, n, count;
  if (scanf("%lu %lu %lu %lu", &scheme, &num_polys, &n, &count) != 4) return 2;
  std::vector<size_t> lens(num_polys, n), poly(count);
  std::vector<unsigned char> points(32 * count, 0), values(32 * count, 0);
  for (size_t i = 0; i < count; ++i) {
    unsigned long p, x, v;
    if (scanf("%lu %lu %lu", &p, &x, &v) != 3) return 2;
    poly[i] = p;
    memcpy(&points[32 * i], &x, sizeof x);
    memcpy(&values[32 * i], &v, sizeof v);
  }
  Openings o;
  o.poly = poly.data(), o.points = points.data(), o.values = values.data(), o.count = count;
  auto less = [](const unsigned char* a, const unsigned char* b) {
    for (int i = 31; i >= 0; --i)
      if (a[i] != b[i]) return a[i] < b[i];
    return false;
  };
  Plan plan;
  if (!make_plan((int)scheme, o, lens.data(), num_polys, n, less, &plan)) return puts("refused"), 0;
  std::vector<uint64_t> flat(flat_words(plan, 32));
  flatten(plan, o, flat.data());
  for (uint64_t w : flat) printf("%lu ", (unsigned long)w);
  puts("");
  return 0;
}
"""


def test_grouping_under_sanitizers(tmp_path, readings):
    """A stand-alone program (its own main, nothing preloaded) groups the
    fixture's index / point pattern under ASan + UBSan and prints the flat
    plan; it equals the reference's."""
    src, exe = tmp_path / "plan_main.cc", tmp_path / "plan_main"
    src.write_text(MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", HEADER_DIR, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for reading, (lens, openings) in readings.items():
        ids = {x: k + 1 for k, x in enumerate(sorted({x for _, x, _ in openings}))}  # order-preserving small ids
        vals = {v: k + 1 for k, v in enumerate(sorted({v for _, _, v in openings}))}
        small = [(i, ids[x], vals[v]) for i, x, v in openings]
        for scheme, sid in ((R.GWC, 0), (R.SHPLONK, 1)):
            text = f"{sid} {len(lens)} 16 {len(small)}\n" + "".join(f"{i} {x} {v}\n" for i, x, v in small)
            run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
            assert run.returncode == 0, run.stderr
            want = R.plan(scheme, lens, 16, small)
            flat = [len(want)]
            for pts, polys in want:
                flat += [len(pts)] + [w for x in pts for w in (x, 0, 0, 0)] + [len(polys)] + polys
            assert [int(w) for w in run.stdout.split()] == flat, (reading, scheme)
    # a clash of claimed values and an index out of range are refused here too
    for text in ("1 1 16 2\n0 1 1\n0 1 2\n", "0 1 16 1\n1 1 1\n"):
        run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.strip() == "refused", run.stderr
