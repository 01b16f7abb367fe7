#!/usr/bin/env python3
"""FRI opening probe over BabyBear / BabyBear4, device-resident, at the shape of
the LDE and commit figures (2^20 x 100 trace, log_blowup 1, shift 31) with two
opening points:

  lde_commit        CosetLDEBatch followed by the bit-reversed build (what
                    TwoAdicFRI::Commit costs in the same run, for comparison)
  reduced_openings  begin + add_round on the extension where Commit left it:
                    inverse denominators, interpolation of the block, the
                    alpha-reduced rows and the accumulation.  The share of the
                    HBM rate counts the matrix's bytes once over the time.
  commit_phase      every commit (tree + root to the host) and fold down to
                    2^log_blowup values, with fixed betas
  queries           100 answer_query calls at spread indices

The extension is honest, so the final values must all be equal: that is checked
before anything is timed.  Every figure is the best of `--reps` runs timed with
device events around the calls (the calls that hand data to the host wait
inside); all samples are recorded.  Writes profiles/fri/probe.json and prints
the same JSON line; fails without a GPU.

    python tools/fri_probe.py [-k 20] [-b 100] [--reps 5] [--out profiles/fri/probe.json]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", type=int, default=20)
    ap.add_argument("-b", type=int, default=100)
    ap.add_argument("--points", type=int, default=2)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri", "probe.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fri_probe: no GPU")
    from tachyon_amd import params
    from tachyon_amd.fri import FriOpening
    from tachyon_amd.ntt import IcicleNTT, IcicleNTTOptions
    from tachyon_amd.poseidon2 import FieldMerkleTree, mul_rate

    p, cols, shift, log_blowup = params.BABY_BEAR, args.b, 31, 1
    rows = 1 << args.k
    n = rows << log_blowup
    gen = params.baby_bear_mont(params.baby_bear_root_of_unity(n)).to_bytes(4, "little")
    ntt = IcicleNTT("baby_bear")
    assert ntt.init(gen, IcicleNTTOptions(are_inputs_on_device=1, are_outputs_on_device=1, is_async=1))
    stream_handle = ntt.stream
    stream = torch.cuda.ExternalStream(stream_handle)
    tree = FieldMerkleTree("horizen", stream_handle)
    fri = FriOpening(log_blowup, "horizen", stream_handle)

    rng = random.Random(20)

    def ext_bytes():
        return b"".join(rng.randrange(p).to_bytes(4, "little") for _ in range(4))

    alpha = ext_bytes()
    points = [ext_bytes() for _ in range(args.points)]
    betas = [ext_bytes() for _ in range(32)]

    x = torch.randint(0, p, (rows * cols,), dtype=torch.int32, device="cuda")
    lde = torch.empty(n * cols, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def commit():
        return (ntt.coset_lde_batch_ptr(x.data_ptr(), rows, cols, log_blowup, shift, lde.data_ptr())
                and tree.build_ptr([(lde.data_ptr(), n, cols)], bit_reversed=True))

    launches = {}

    def reduce():
        ok = fri.begin(alpha) and fri.add_round_ptr([(lde.data_ptr(), n, cols)], [points]) is not None
        launches["reduced_openings"] = fri.last_launches
        return ok

    def commit_phase():
        step = iter(betas)
        count = [0]

        def on_commit(root):
            count[0] += fri.last_launches
            return next(step)

        roots = fri.commit_phase(on_commit)
        launches["commit_phase"] = count[0] + len(roots)        # every tree's launches and one fold each
        return len(roots) == args.k

    def queries():
        return all(fri.answer_query((q * 2654435761) % n) is not None for q in range(args.queries))

    def timed(call, setup=None):
        """seconds of `call`, best of --reps after a warm-up; setup runs untimed before each"""
        samples = []
        for rep in range(args.reps + 1):
            if setup:
                assert setup()
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert call()
            e1.record(stream)
            e1.synchronize()
            if rep:
                samples.append(e0.elapsed_time(e1) / 1e3)
        return min(samples), samples

    out = {"probe": "fri_baby_bear", "device": torch.cuda.get_device_name(0), "external": "horizen",
           "log_rows": args.k, "cols": cols, "log_blowup": log_blowup, "points": args.points, "reps": args.reps,
           "checks": {}}

    # ---- check: an honest extension folds to a constant
    assert commit() and reduce() and commit_phase()
    final = fri.final_poly()
    out["checks"]["final_values_equal"] = final is not None and final[:16] == final[16:32]
    out["checks"]["num_commits"] = fri.num_commits == args.k
    if not all(out["checks"].values()):
        print(json.dumps(out))
        raise SystemExit("fri_probe: a check failed")

    s, samples = timed(commit)
    out["lde_commit"] = {"seconds": s, "samples": samples}
    s, samples = timed(reduce)
    matrix_bytes = n * cols * 4
    out["reduced_openings"] = {
        "seconds": s, "samples": samples, "launches": launches["reduced_openings"],
        "matrix_bytes": matrix_bytes, "hbm_share_of_8TBps": matrix_bytes / HBM_BYTES_PER_S / s,
        "base_products": n * cols * 4 + (n >> log_blowup) * cols * 4 * args.points,
    }
    s, samples = timed(commit_phase, setup=reduce)
    out["commit_phase"] = {"seconds": s, "samples": samples, "commits": args.k, "launches": launches["commit_phase"]}
    s, samples = timed(queries)
    out["queries"] = {"count": args.queries, "seconds": s, "samples": samples, "launches_per_query": fri.last_launches}
    out["bb31_mul_products_per_second"] = mul_rate(1 << 22, 4096)
    ro = out["reduced_openings"]
    ro["valu_share"] = ro["base_products"] / ro["seconds"] / out["bb31_mul_products_per_second"]

    fri.close()
    tree.close()
    ntt.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
