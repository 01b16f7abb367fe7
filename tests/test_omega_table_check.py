"""The omega power tables and the upload's section packer (csrc/common/
omega_table.h, sections.h) on the host alone: check/omega_table_check.cc, a
stand-alone program with its own main, built under the address and undefined
behaviour sanitizers with nothing preloaded.  Runs without a GPU."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tachyon_amd", "csrc")


def test_omega_table_check_under_sanitizers(tmp_path):
    """The tables' size, A B C = omega^j at the seams of the three tables for
    n around 256 and 65536, and the packer's offsets against the drivers' sums."""
    exe = tmp_path / "omega_table_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", str(exe),
                        os.path.join(CSRC, "check", "omega_table_check.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "omega_table_check ok", run.stdout + run.stderr


def test_makefile_builds_the_check():
    r = subprocess.run(["make", "-s", "-n", "-C", CSRC, "../bin/omega_table_check"], capture_output=True, text=True)
    assert r.returncode == 0 and "omega_table_check.cc" in r.stdout, r.stderr
