"""The bench.py output contract, checked on the newest committed bench line
(profiles/<round>/bench_line*.json, the line of a `bench.py --full` run on an
MI355X): the keys the driver and the judge read, a roofline object with its
fraction consistent, and the CPU baseline beside it.  No GPU needed, except
for the one plain run at a small size (marked gpu)."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def newest_bench_line():
    # newest round tag first (file mtimes are the checkout's); the 1-GPU
    # default-run lines only (multi-rank rehearsals carry no CPU baseline)
    import re

    def order(f):  # run order: r05z < r05aa < r05ab (as bench.pmc_traffic)
        m = re.fullmatch(r"r(\d+)([a-z]*)", os.path.basename(os.path.dirname(f)))
        return (int(m.group(1)), len(m.group(2)), m.group(2), f) if m else (-1, 0, "", f)

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "bench_line*.json")), key=order)
    if not files:
        pytest.skip("no committed bench line")
    for path in reversed(files):
        if "rehearsal" in os.path.basename(path):
            continue
        text = open(path).read().strip()
        if text.startswith("{"):
            d = json.loads(text.splitlines()[-1])
            if d.get("n_gpus") == 1:
                return path, d
    pytest.skip("no parsable bench line")


def test_bench_line_contract():
    path, d = newest_bench_line()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, (path, k)
    assert d["higher_is_better"] is True and d["unit"] == "scalars/s"
    assert d["scaling"] in ("weak", "strong")
    # value = the 2^msm_log_n scalars of one step / the step time
    n = 1 << d["config"]["msm_log_n"]
    assert abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1


def test_bench_cli_parses_without_gpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "--gpus" in out.stdout and "--steps" in out.stdout
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


# the objects of a --full line that a plain run leaves out
FULL_ONLY = ("roofline", "valu_roofline", "msm_phase_ms", "msm_sweep", "projected_scaling", "non_uniform", "ntt",
             "bls12_381", "groth16", "host_resident", "cpu_baseline", "consistent_with_1gpu")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_its_result(tmp_path):
    """A plain run (no --full) at a small size: the line carries the headline
    keys and none of the legs behind --full, --steps is the number of timed
    steps, and --dump-outputs writes the last step's affine point, which equals
    the oracle's MSM of the same seeded inputs."""
    import numpy as np
    torch = pytest.importorskip("torch")
    import bench
    from oracle import oracle as O
    from tachyon_amd import msm as M
    log_n, steps = 12, 3
    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--log-n", str(log_n), "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "consistent_across_steps"):
        assert k in d, k
    assert not [k for k in FULL_ONLY if k in d]
    assert d["steps"] == steps and d["warmup"] == 1 and d["consistent_across_steps"] is True
    assert d["higher_is_better"] is True and d["unit"] == "scalars/s" and d["dtype"] == "u32"
    n = 1 << log_n
    assert d["ms_per_step"] > 0 and abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert sorted(os.listdir(dump)) == ["msm_result.npy"]
    got = np.load(dump / "msm_result.npy")
    assert got.dtype == np.float64 and got.shape == (16,)
    d_b = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    d_s = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    M.gen_bases("bn254_g1", bench.SEED, n, 1 << 10, d_b.data_ptr())
    M.gen_scalars("bn254_fr", bench.SEED, n, d_s.data_ptr())
    torch.cuda.synchronize()
    expect, _ = O.msm("bn254_g1", d_b.cpu().numpy().tobytes(), d_s.cpu().numpy().tobytes())
    assert got.astype("<u4").tobytes() == expect


def test_pmc_traffic_takes_the_newest_run(tmp_path, monkeypatch):
    """bench.pmc_traffic reads the newest committed profile in run order
    (r05z < r05aa < r05ab: spreadsheet-column suffixes), not the
    lexicographically last directory."""
    import json
    import bench
    for run, gb in (("r05y", 1.0), ("r05z", 2.0), ("r05ab", 3.0), ("r04zz", 9.0)):
        d = tmp_path / "profiles" / run
        d.mkdir(parents=True)
        (d / "pmc_traffic.json").write_text(json.dumps({"k": {"traffic_bytes": gb * 1e9}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    traffic, src, _ = bench.pmc_traffic("k")
    assert traffic == 3.0 and src.endswith("r05ab/pmc_traffic.json")
