"""The C-ABI guards (tachyon_amd/csrc/capi/capi_guard.h): host code, so it
runs without a GPU.  check/capi_guard_check.cc, a stand-alone program with its
own main that includes nothing of the project but that header, is built with a
plain host compiler under the address and undefined-behaviour sanitizers and
run: guarded() and guarded_report() return the body's value or the fallback,
the report is the exact line on stderr, and the aborting guard passes a value
through.  The abort path is not exercised."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tachyon_amd", "csrc")
CHECK = os.path.join(CSRC, "check", "capi_guard_check.cc")


def test_guard_check_under_sanitizers(tmp_path):
    exe = tmp_path / "capi_guard_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", str(exe), CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "capi_guard_check ok" and run.stderr == "", run.stdout + run.stderr


def test_one_guard_in_the_tree():
    """die() and GUARD_END are defined once, in capi_guard.h, which stays
    host-only; the check program includes no other project header."""
    defs = {"die": [], "GUARD_END": []}
    for d, _, files in os.walk(CSRC):
        for f in files:
            if not f.endswith((".h", ".hip", ".cc")):
                continue
            text = open(os.path.join(d, f)).read()
            if re.search(r"^\s*(\[\[noreturn\]\]\s*)?(inline\s+|static\s+)*void\s+die\s*\(", text, re.M):
                defs["die"].append(f)
            if re.search(r"^\s*#\s*define\s+GUARD_END\b", text, re.M):
                defs["GUARD_END"].append(f)
    assert defs == {"die": ["capi_guard.h"], "GUARD_END": ["capi_guard.h"]}, defs
    guard = open(os.path.join(CSRC, "capi", "capi_guard.h")).read()
    assert "hip" not in [m.split("/")[0] for m in re.findall(r'#include\s+[<"]([^>"]+)[>"]', guard)]
    quoted = re.findall(r'#include\s+"([^"]+)"', open(CHECK).read())
    assert quoted == ["../capi/capi_guard.h"], quoted
