"""The permuted lookup columns' entry points without a GPU: declared in
include/tachyon_mi355x.h, exported by the library, bound by tachyon_amd._lib,
every one that can throw behind the common guard, and the refusals -- decided
before any GPU call -- through the Python binding on host columns."""
import os
import re
import subprocess

import pytest

import lookup_permute_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tachyon_mi355x.h")
LIB = os.path.join(ROOT, "tachyon_amd", "libtachyon_mi355x.so")
CAPI = os.path.join(ROOT, "tachyon_amd", "csrc", "capi", "capi_lookup_permute.hip")
ENTRIES = ["tachyon_mi355x_lookup_permute_pairs", "tachyon_mi355x_lookup_permute_work_bytes",
           "tachyon_mi355x_lookup_permute_last_timings"]
F = R.field("bn254_fr")


@pytest.fixture(scope="module")
def libpath():
    if not os.path.exists(LIB):
        pytest.skip("libtachyon_mi355x.so not built (run __graft_entry__.build())")
    return LIB


def test_declared_exported_and_bound(libpath):
    text = open(HEADER).read()
    declared = set(re.findall(r"TACHYON_C_EXPORT[^;(]*?\b(tachyon_\w+)\s*\(", text, re.S))
    assert set(ENTRIES) <= declared
    assert re.search(r"typedef struct \{\s*const void\* input;\s*const void\* table;\s*\} tachyon_mi355x_lookup_pair;",
                     text)
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(ENTRIES) <= exported
    from tachyon_amd._lib import SIGNATURES, lib
    assert set(ENTRIES) <= {n for n, _, _ in SIGNATURES}
    for name in ENTRIES:
        assert getattr(lib(), name).argtypes is not None


def test_entries_run_under_the_guard():
    """Every entry point whose body can throw returns through guarded_report,
    behind the host-only validation; the one that cannot (a copy under a
    mutex) has no call that allocates or touches the GPU."""
    text = open(CAPI).read()
    # every definition ends with a closing brace and a blank line
    bodies = dict(re.findall(r"^(?:int|size_t|void) (tachyon_mi355x_lookup_permute_\w+)\([^{]*\{(.*?)\}\n\n", text,
                             re.S | re.M))
    assert sorted(bodies) == sorted(ENTRIES)
    for name in ("pairs", "work_bytes"):
        body = bodies["tachyon_mi355x_lookup_permute_" + name]
        assert "return guarded_report(__func__" in body, name
        outside = body[:body.index("guarded_report")]
        assert "require_gpu" not in outside and "LookupPermute" not in outside and "run_" not in outside, name
    body = bodies["tachyon_mi355x_lookup_permute_pairs"]
    assert body.index("lp_validate::check_permute_pairs") < body.index("guarded_report")
    assert body.index("count == 0") < body.index("guarded_report")  # nothing to do: no GPU call
    body = bodies["tachyon_mi355x_lookup_permute_last_timings"]
    assert not re.search(r"hip|new |std::vector|require_gpu", body)
    assert "GUARD_BEGIN" not in text  # report and return 0: these entry points never abort


def test_refusals_need_no_gpu(libpath):
    """Host columns, so nothing here touches a device: a refused call returns
    None before the library looks for one."""
    from tachyon_amd import lookup_permute as LP
    from tachyon_amd import plonk
    assert LP._Columns is plonk._Columns and LP._ptr is plonk._ptr  # reused, not copied
    assert set(LP.last_timings()) == set(LP.PHASES) and len(LP.PHASES) == 4
    n, u = 16, 10
    A, S = R.encode(F, range(n)), R.encode(F, range(n))
    blinds = bytes(32 * 2 * (n - u))
    for n_, u_ in ((n, 0), (n, n), (n, n + 3)):
        assert LP.permute_pairs("bn254_fr", n_, u_, [(A, S)], bytes(32 * 2 * max(0, n_ - u_))) is None
    assert LP.permute_pairs("bn254_fr", 12, 5, [(bytes(32 * 12), bytes(32 * 12))], bytes(32 * 14)) is None
    assert LP.permute_pairs("bn254_fr", 1, 0, [(bytes(32), bytes(32))], bytes(64)) is None
    assert LP.permute_pairs("bn254_fr", n, u, [(None, S)], blinds) is None
    assert LP.permute_pairs("bn254_fr", n, u, [(A, None)], blinds) is None
    assert LP.permute_pairs("bn254_fr", n, u, [(A, S), (A, None)], blinds * 2) is None
    # the blind count: 2 (n - u) per pair, neither one column's nor one value off
    assert LP.permute_pairs("bn254_fr", n, u, [(A, S)], blinds[32:]) is None
    assert LP.permute_pairs("bn254_fr", n, u, [(A, S)], blinds + bytes(32)) is None
    assert LP.permute_pairs("bn254_fr", n, u, [(A, S)], blinds[:32 * (n - u)]) is None
    assert LP.permute_pairs("bn254_fr", n, u, [(A, S)], [blinds, blinds]) is None
    assert LP.permute_pairs("bn254_fr", n, u, [], b"") == ([], [], [])  # nothing to do: no refusal, no GPU call
    assert LP.permute_pairs("bn254_fr", n, u, [], blinds) is None


def test_the_c_entry_refuses_on_host_pointers(libpath):
    """What the binding cannot express: the field, null arrays, null and
    overlapping outputs, straight through the C entry point."""
    import ctypes

    from tachyon_amd import lookup_permute as LP
    from tachyon_amd._lib import lib
    n, u = 16, 10
    entry = lib().tachyon_mi355x_lookup_permute_pairs
    cols = [ctypes.create_string_buffer(32 * n) for _ in range(2)]
    outs = [ctypes.create_string_buffer(b"\xAB" * (32 * n), 32 * n) for _ in range(2)]
    blinds = ctypes.create_string_buffer(32 * 2 * (n - u))
    pairs = (LP.LookupPair * 1)()
    pairs[0].input, pairs[0].table = ctypes.addressof(cols[0]), ctypes.addressof(cols[1])

    def ptrs(b):
        """a one-pointer array: to a buffer, to an address, or null"""
        return (ctypes.c_void_p * 1)(b if b is None or isinstance(b, int) else ctypes.addressof(b))

    out_a, out_s = ptrs(outs[0]), ptrs(outs[1])
    for field in (1, 3, -1):
        assert entry(field, n, u, pairs, 1, blinds, out_a, out_s, None) == 0
    assert entry(0, n, u, None, 1, blinds, out_a, out_s, None) == 0
    assert entry(0, n, u, pairs, 1, None, out_a, out_s, None) == 0
    assert entry(0, n, u, pairs, 1, blinds, None, out_s, None) == 0
    assert entry(0, n, u, pairs, 1, blinds, out_a, None, None) == 0
    assert entry(0, n, u, pairs, 1, blinds, ptrs(None), out_s, None) == 0
    assert entry(0, n, u, pairs, 1, blinds, out_a, ptrs(None), None) == 0
    assert entry(0, n, u, pairs, 1, blinds, out_a, out_a, None) == 0  # S' is A'
    assert entry(0, n, u, pairs, 1, blinds, out_a, ptrs(ctypes.addressof(outs[0]) + 32 * (n - 1)), None) == 0
    assert entry(0, n, u, pairs, 1, blinds, ptrs(cols[0]), out_s, None) == 0  # A' is A
    assert entry(0, n, u, pairs, 1, blinds, out_a, ptrs(cols[0]), None) == 0  # S' is A
    assert entry(0, n, u, pairs, 1, blinds, out_a, ptrs(ctypes.addressof(cols[1]) + 32), None) == 0
    assert entry(0, 1 << 31, u, pairs, 1, blinds, out_a, out_s, None) == 0
    assert all(o.raw == b"\xAB" * (32 * n) for o in outs)
    assert entry(0, n, u, None, 0, None, None, None, None) == 1  # count = 0
