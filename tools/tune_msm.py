#!/usr/bin/env python3
"""Window-size sweep for the MSM (device-resident BN254 G1 inputs).

  python tools/tune_msm.py --log-n 26 --c 16 18 20 21 22
  python tools/tune_msm.py --log-n 26 --c 0 --mixed 0 12 13 14
Prints per-phase device time (HIP events) for each window size; --mixed W
sweeps W windows of two widths (set_mixed_windows; 0 = the size's default
plan, which --variants 134217728 keeps uniform) beside the uniform --c.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[26])
    ap.add_argument("--c", type=int, nargs="+", default=[0])
    ap.add_argument("--mixed", type=int, nargs="+", default=[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--non-uniform", action="store_true")
    ap.add_argument("--variants", type=int, nargs="+", default=[0])
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--curve", default="bn254_g1")
    args = ap.parse_args()
    import torch
    from tachyon_amd import msm as M
    for lg in args.log_n:
        n = 1 << lg
        from tachyon_amd._lib import CURVE_INFO
        pb, sf = CURVE_INFO[args.curve]
        d_b = torch.empty(n * pb, dtype=torch.uint8, device="cuda")
        d_s = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        M.gen_bases(args.curve, 1, n, 1024, d_b.data_ptr())
        if args.non_uniform:
            M.gen_scalars(sf, 1, 1, d_s.data_ptr())
            d_s.view(n, 32)[:] = d_s[:32]
        else:
            M.gen_scalars(sf, 1, n, d_s.data_ptr())
        torch.cuda.synchronize()
        m = M.VariableBaseMSMGpu(args.curve)
        ref = None
        # every uniform c (with the default layout), then every mixed W (no forced bits)
        layouts = [(c, 0) for c in args.c] + [(0, w) for w in args.mixed if w]
        for c, mixed, var in [(c, w, v) for _ in range(args.rounds) for c, w in layouts for v in args.variants]:
            if m.mixed_windows != mixed:
                m.set_mixed_windows(0)
            m.set_window_bits(c)
            if mixed:
                m.set_mixed_windows(mixed)
            m.set_variant(var)
            m.set_profile(True)
            res = m.run(d_b, d_s)
            ref = ref or res
            times, walls = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                r = m.run(d_b, d_s)
                walls.append((time.perf_counter() - t0) * 1e3)
                times.append(m.last_timings())
                assert r == ref or (var & 64), "result changed"
            best = min(range(args.reps), key=lambda i: walls[i])
            W, is_mixed = m.plan_windows(n), m.last_schedule().get("mixed_windows", False)
            c_def, w_def = M.plan(args.curve, n)
            # the bits of the (narrow) windows; None where variant bit 27 leaves the size's default plan
            c_run = c or (M.mixed_layout(args.curve, W)["c_lo"] if is_mixed else c_def if w_def == W else None)
            print(json.dumps({"curve": args.curve, "log_n": lg, "c": c_run, "windows": W, "mixed": is_mixed,
                              "variant": var, "wall_ms": round(walls[best], 3),
                              **{k: round(v, 3) for k, v in times[best].items()}}), flush=True)
        m.close()


if __name__ == "__main__":
    main()
