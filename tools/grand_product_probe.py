#!/usr/bin/env python3
"""Grand-product probe over BN254 Fr, device-resident columns: the permutation
argument's Z for one circuit as a chain of 3 jobs, at n = 2^20 and 2^22 rows
with 1, 2 and 4 columns per job (numerator v + beta delta^i omega^j + gamma,
denominator v + beta sigma + gamma; Z written into CUDA tensors).

Per shape it records the three passes of tachyon_mi355x_grand_product_chains
-- ratios (the row kernel and the tile inversions), carries, apply -- in milliseconds from the library's own stream
events (tachyon_mi355x_grand_product_last_timings), best of `--reps` with every
sample kept, and beside them the bytes the passes must move: every input
column once per job (c value and c sigma columns), the ratio written and read
once, Z written once; and that total over the passes' time as a share of the
HBM rate.  It also records KZG.commit_lagrange on one of the Z tensors at the
same size, so that the step's share of "make Z and commit it" can be read off.

Writes profiles/grand_product/probe.json and prints the same JSON line; fails
without a GPU.

    python tools/grand_product_probe.py [--log-n 20 22] [--cols 1 2 4] [--reps 5] [--no-commit]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
FIELD = "bn254_fr"
JOBS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--cols", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-commit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grand_product", "probe.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grand_product_probe: no GPU")
    from tachyon_amd import params as P
    from tachyon_amd import plonk
    from tachyon_amd.kzg import KZG

    r = P.FIELDS[FIELD][0]

    def mont(x):
        return P.mont(x, r, 4).to_bytes(32, "little")

    gen = torch.Generator(device="cuda").manual_seed(47)

    def column(n):  # canonical Montgomery bytes: 253 random bits per element
        t = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen)
        t[:, 31] &= 0x1F
        return t.reshape(-1)

    result = {"field": FIELD, "jobs_per_chain": JOBS, "tile_rows": plonk.tile_rows(), "walk_tiles": plonk.walk_tiles(),
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps, "shapes": []}
    beta, gamma = mont(0xBE7A), mont(0x6A33A)
    for log_n in args.log_n:
        n = 1 << log_n
        u = n - 6
        omega = mont(pow(5, (r - 1) // n, r))
        blinds = [b"".join(mont(1000 + 7 * k + j) for j in range(n - u - 1)) for k in range(JOBS)]
        most = JOBS * max(args.cols)
        values = [column(n) for _ in range(most)]
        sigmas = [column(n) for _ in range(most)]
        out = [torch.empty(32 * n, dtype=torch.uint8, device="cuda") for _ in range(JOBS)]
        torch.cuda.synchronize()
        commit_ms = None
        for cols in args.cols:
            m = JOBS * cols
            call = lambda: plonk.permutation_grand_products([values[:m]], sigmas[:m], beta, gamma, cols + 2, n, u,
                                                            omega, blinds=blinds, out=out)
            first = call()  # warm-up
            assert first is not None and len(first[0][0]) == JOBS
            samples, wall = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                again = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                assert again[1] == first[1]
                samples.append(plonk.last_timings())
            best = {ph: min(s[ph] for s in samples) for ph in ("ratios", "carries", "apply")}
            e = 32 * n
            moved = {"inputs_once": JOBS * 2 * cols * e, "ratio_write_and_read": JOBS * 2 * e, "z_write": JOBS * e}
            total = sum(moved.values())
            passes_ms = sum(best.values())
            rec = {"log_n": log_n, "usable_rows": u, "columns_per_job": cols, "ms": best, "passes_ms": passes_ms,
                   "samples_ms": samples, "call_ms": min(wall), "call_samples_ms": wall, "bytes": moved,
                   "bytes_total": total, "hbm_share": total / (passes_ms * 1e-3) / HBM_BYTES_PER_S}
            result["shapes"].append(rec)
            print(f"[grand_product_probe] 2^{log_n} x {cols}: {json.dumps(best)}", file=sys.stderr, flush=True)
        if not args.no_commit:
            kzg = KZG("bn254_g1")
            kzg.unsafe_setup(n, mont(0x1234567890ABCDEF))
            assert kzg.commit_lagrange(out[0]) is not None  # warm-up
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                kzg.commit_lagrange(out[0])
                ts.append((time.perf_counter() - t0) * 1e3)
            kzg.close()
            commit_ms = min(ts)
            for rec in result["shapes"]:
                if rec["log_n"] == log_n:
                    rec["commit_lagrange_one_z_ms"] = commit_ms
                    rec["commit_lagrange_samples_ms"] = ts
                    # per Z polynomial: its share of the passes against one commitment
                    per_z = rec["passes_ms"] / JOBS
                    rec["z_share_of_make_and_commit"] = per_z / (per_z + commit_ms)
        del values, sigmas, out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
