#!/usr/bin/env python3
"""Log-derivative lookup probe over BN254 Fr, device-resident columns: one
lookup with K = 1, 2 and 4 compressed input columns at n = 2^20 and 2^22 rows.
The table is a column of distinct random values, every input row holds the
value of a random usable table row (no miss), m and phi are written into CUDA
tensors and m stays on the device between the two calls.

Per shape it records the phases of tachyon_mi355x_log_lookup_m_polys (sort,
count) and tachyon_mi355x_log_lookup_grand_sums (A terms and tile inversions,
B carries, C apply) in milliseconds from the library's own stream events
(tachyon_mi355x_log_lookup_last_timings), best of `--reps` with every sample
kept; each whole call on the host clock; the count phase again with every
input row equal (all adds of a column on one counter); and beside them the
bytes each phase must move and its field products per row (the formulas are in
DESIGN 4.9).  It also records KZG.commit_lagrange on the phi tensor at the same
size, so that the step's share of "make m and phi and commit them" can be read
off.

Writes profiles/log_lookup/probe.json and prints the same JSON line; fails
without a GPU.

    python tools/log_lookup_probe.py [--log-n 20 22] [--inputs 1 2 4] [--reps 5] [--no-commit]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
FIELD = "bn254_fr"
M_PHASES = ("sort", "count")
SUM_PHASES = ("sums_a", "sums_b", "sums_c")


def must_move(n, u, K, tile):
    """Bytes each phase cannot avoid, by phase: what it reads once and writes once."""
    e, tiles = 32, -(-n // tile)
    return {"sort": e * u + e * u + 4 * u,  # the table in; the sorted keys and the permutation out
            # the inputs in, log2(u) probes of a 16-byte key half each, the counters, m out
            "count": K * e * u + K * u * math.ceil(math.log2(u)) * 16 + 2 * 4 * u + e * n,
            "sums_a": (K + 2) * e * u + e * u,  # inputs, table, m in; q out
            "sums_b": 2 * e * tiles,
            "sums_c": e * u + e * n}  # q in; phi out


def products_per_row(K, tile):
    """Field products per usable row, by phase (a Montgomery reduction alone counts one half)."""
    scans = 2 * 7 / 4  # two product scans of 6 shuffle steps and the wave totals, per thread of 4 rows
    return {"sort": 0.5, "count": 0.5 * K + 1.0, "sums_a": (2 * K + 3) + 5 + scans + 381 / tile, "sums_b": 0.0,
            "sums_c": 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--inputs", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-commit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_lookup", "probe.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("log_lookup_probe: no GPU")
    from tachyon_amd import log_lookup as LL
    from tachyon_amd import params as P
    from tachyon_amd.kzg import KZG

    r = P.FIELDS[FIELD][0]

    def mont(x):
        return P.mont(x, r, 4).to_bytes(32, "little")

    gen = torch.Generator(device="cuda").manual_seed(49)

    def column(n):  # canonical Montgomery bytes: 253 random bits per element
        t = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen)
        t[:, 31] &= 0x1F
        return t

    tile = LL.tile_rows()
    result = {"field": FIELD, "tile_rows": tile, "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps, "shapes": []}
    beta = mont(0xBE7A)
    for log_n in args.log_n:
        n = 1 << log_n
        u = n - 6
        blinds = [b"".join(mont(1000 + j) for j in range(n - u - 1))]
        table = column(n)
        most = max(args.inputs)
        rows = [torch.randint(0, u, (n,), device="cuda", generator=gen) for _ in range(most)]
        inputs = [table[idx].reshape(-1) for idx in rows]
        equal = table[17].repeat(n)  # every row the value of table row 17
        table = table.reshape(-1)
        m_out = [torch.empty(32 * n, dtype=torch.uint8, device="cuda")]
        phi_out = [torch.empty(32 * n, dtype=torch.uint8, device="cuda")]
        torch.cuda.synchronize()

        def timed(call, phases):
            first = call()  # warm-up
            assert first is not None
            samples, wall = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                again = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                assert again[1] == first[1]
                ms = LL.last_timings()
                samples.append({ph: ms[ph] for ph in phases})
            return first, {ph: min(s[ph] for s in samples) for ph in phases}, samples, wall

        for K in args.inputs:
            lookups = [(inputs[:K], table)]
            (_, misses), m_best, m_samples, m_wall = timed(
                lambda: LL.m_polys(FIELD, n, u, lookups, out=m_out), M_PHASES)
            assert misses == [0]
            (_, totals), s_best, s_samples, s_wall = timed(
                lambda: LL.grand_sums(FIELD, n, u, beta, lookups, m_out, blinds, out=phi_out), SUM_PHASES)
            assert totals == [bytes(32)]  # the lookup balances
            best = dict(m_best, **s_best)
            moved, prods = must_move(n, u, K, tile), products_per_row(K, tile)
            rec = {"log_n": log_n, "usable_rows": u, "inputs": K, "ms": best, "phases_ms": sum(best.values()),
                   "m_polys_samples_ms": m_samples, "grand_sums_samples_ms": s_samples,
                   "m_polys_call_ms": min(m_wall), "m_polys_call_samples_ms": m_wall,
                   "grand_sums_call_ms": min(s_wall), "grand_sums_call_samples_ms": s_wall,
                   "must_move_bytes": moved, "products_per_row": prods,
                   "hbm_share": {ph: moved[ph] / (best[ph] * 1e-3) / HBM_BYTES_PER_S for ph in best},
                   "products_per_s": {ph: prods[ph] * u / (best[ph] * 1e-3) for ph in best}}
            # every input row the same value: K * u adds on one counter
            hot = [([equal] * K, table)]
            (_, misses), h_best, h_samples, h_wall = timed(lambda: LL.m_polys(FIELD, n, u, hot, out=m_out), M_PHASES)
            assert misses == [0]
            rec["all_equal_inputs"] = {"ms": h_best, "samples_ms": h_samples, "call_ms": min(h_wall)}
            result["shapes"].append(rec)
            print(f"[log_lookup_probe] 2^{log_n} x {K}: {json.dumps(best)} all equal: {json.dumps(h_best)}",
                  file=sys.stderr, flush=True)
        if not args.no_commit:
            kzg = KZG("bn254_g1")
            kzg.unsafe_setup(n, mont(0x1234567890ABCDEF))
            assert kzg.commit_lagrange(phi_out[0]) is not None  # warm-up
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                kzg.commit_lagrange(phi_out[0])
                ts.append((time.perf_counter() - t0) * 1e3)
            kzg.close()
            for rec in result["shapes"]:
                if rec["log_n"] == log_n:
                    rec["commit_lagrange_one_column_ms"] = min(ts)
                    rec["commit_lagrange_samples_ms"] = ts
                    # m and phi made, against m and phi made and both committed
                    made = rec["m_polys_call_ms"] + rec["grand_sums_call_ms"]
                    rec["share_of_make_and_commit"] = made / (made + 2 * min(ts))
        del table, inputs, rows, equal, m_out, phi_out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
