"""The log-derivative lookup's entry points without a GPU: declared in
include/tachyon_mi355x.h, exported by the library, bound by tachyon_amd._lib,
every one that can throw behind the common guard, and the refusals -- decided
before any GPU call -- through the Python binding on host columns."""
import os
import re
import subprocess

import pytest

import log_lookup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tachyon_mi355x.h")
LIB = os.path.join(ROOT, "tachyon_amd", "libtachyon_mi355x.so")
CAPI = os.path.join(ROOT, "tachyon_amd", "csrc", "capi", "capi_log_lookup.hip")
ENTRIES = ["tachyon_mi355x_log_lookup_m_polys", "tachyon_mi355x_log_lookup_grand_sums",
           "tachyon_mi355x_log_lookup_tile_rows", "tachyon_mi355x_log_lookup_work_bytes",
           "tachyon_mi355x_log_lookup_last_timings"]
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
    assert re.search(r"typedef struct \{[^}]*inputs;[^}]*num_inputs;[^}]*table;\s*\} tachyon_mi355x_log_lookup;", text)
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(ENTRIES) <= exported
    from tachyon_amd._lib import SIGNATURES, lib
    assert set(ENTRIES) <= {n for n, _, _ in SIGNATURES}
    for name in ENTRIES:
        assert getattr(lib(), name).argtypes is not None


def test_entries_run_under_the_guard():
    """Every entry point whose body can throw returns through guarded_report,
    behind the host-only validation; the two that cannot (a constant, a copy
    under a mutex) have no call that allocates or touches the GPU."""
    text = open(CAPI).read()
    # every definition ends with a closing brace and a blank line
    bodies = dict(re.findall(r"^(?:int|size_t|void) (tachyon_mi355x_log_lookup_\w+)\([^{]*\{(.*?)\}\n\n", text,
                             re.S | re.M))
    assert sorted(bodies) == sorted(ENTRIES)
    for name in ("m_polys", "grand_sums", "work_bytes"):
        body = bodies["tachyon_mi355x_log_lookup_" + name]
        assert "return guarded_report(__func__" in body, name
        outside = body[:body.index("guarded_report")]
        assert "require_gpu" not in outside and "LogLookup" not in outside and "run_" not in outside, name
    for name, check in (("m_polys", "check_m_polys"), ("grand_sums", "check_grand_sums")):
        body = bodies["tachyon_mi355x_log_lookup_" + name]
        assert body.index("ll_validate::" + check) < body.index("guarded_report"), name
    for name in ("tile_rows", "last_timings"):
        body = bodies["tachyon_mi355x_log_lookup_" + name]
        assert not re.search(r"hip|new |std::vector|require_gpu", body), name
    assert "GUARD_BEGIN" not in text  # report and return 0: these entry points never abort


def test_refusals_need_no_gpu(libpath):
    """Host columns, so nothing here touches a device: a refused call returns
    None before the library looks for one."""
    from tachyon_amd import log_lookup as LL
    from tachyon_amd import plonk
    assert LL._Columns is plonk._Columns and LL._ptr is plonk._ptr  # reused, not copied
    assert LL.tile_rows() > 0 and LL.tile_rows() % 64 == 0
    assert set(LL.last_timings()) == set(LL.PHASES)
    n, u = 16, 10
    col = [R.encode(F, range(k, k + n)) for k in range(3)]
    beta, blinds = F.to_bytes(5), bytes(32 * (n - u - 1))
    good = [([col[0]], col[1])]
    for n_, u_ in ((n, 0), (n, n), (n, n + 3)):
        assert LL.m_polys("bn254_fr", n_, u_, good) is None
        assert LL.grand_sums("bn254_fr", n_, u_, beta, good, [col[2]], bytes(32 * max(0, n_ - u_ - 1))) is None
    odd = [([bytes(32 * 12)], bytes(32 * 12))]
    assert LL.m_polys("bn254_fr", 12, 5, odd) is None
    assert LL.grand_sums("bn254_fr", 12, 5, beta, odd, [bytes(32 * 12)], bytes(32 * 6)) is None
    for bad in ([([], col[1])], [([col[0], None], col[1])], [([col[0]], None)]):
        assert LL.m_polys("bn254_fr", n, u, bad) is None
        assert LL.grand_sums("bn254_fr", n, u, beta, bad, [col[2]], blinds) is None
    assert LL.grand_sums("bn254_fr", n, u, None, good, [col[2]], blinds) is None
    assert LL.grand_sums("bn254_fr", n, u, beta, good, [None], blinds) is None
    assert LL.grand_sums("bn254_fr", n, u, beta, good, [col[2]], blinds[32:]) is None
    assert LL.grand_sums("bn254_fr", n, u, beta, good, [col[2]], blinds + bytes(32)) is None
    assert LL.m_polys("bn254_fr", n, u, []) == ([], [])  # nothing to do: no refusal, no GPU call
