#!/usr/bin/env python3
"""Quotient probe over BN254 Fr, device-resident polynomials: h(X) of one
circuit at n = 2^20 and 2^22 rows with cs_degree 4 (P = 4 parts), through
tachyon_mi355x_quotient_h_poly.

The workload is synthetic: 4 fixed, 8 advice and 1 instance column; a gate
set of `--blocks` blocks, each the product of `live` sums (column + constant)
squared once and folded into the running value with y (so `live` + 1 values
are live at once) -- in two variants, `live` = fast_slots - 2 (every
intermediate in LDS) and `live` = 2 fast_slots (half of them in the spill
workspace); one permutation of 8 columns (4 products Z) and one lookup.

Per shape and variant it records the phases of the call in milliseconds from
the library's own stream events (tachyon_mi355x_quotient_last_timings), best
of `--reps` by the evaluator's total with every sample kept, and beside them
what the lowered programs do per row (tachyon_mi355x_quotient_program_stats):
field products, column elements read, slots; the evaluator's products per
second against the 138.6 G mulmod/s in-register ceiling of DESIGN, its column
bytes per second against 8 TB/s, and the evaluator's share of the summed
event spans next to the coset transforms.  The spans leave out what every
call does before and after them -- planning on the host, allocating the
buffers, building the domain's tables (a fresh domain per call), the upload --
so the host's wall clock around the whole call is recorded beside them.

Writes profiles/quotient/probe.json and prints the same JSON line; fails
without a GPU.

    python tools/quotient_probe.py [--log-n 20 22] [--blocks 8] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
MULMOD_PER_S = 138.6e9
FIELD = "bn254_fr"
CS_DEGREE = 4
NUM_FIXED, NUM_ADVICE, NUM_INSTANCE, PERM_COLUMNS = 4, 8, 1, 8


def gate_graph(Q, live, blocks):
    g = Q.GraphEvaluator(FIELD)
    rots = [g.add_rotation(r) for r in (0, 1, -1)]
    run, k = (Q.PREVIOUS_VALUE, 0, 0), 0
    for _ in range(blocks):
        vals = []
        for _ in range(live):
            col = (Q.ADVICE, k % NUM_ADVICE, rots[k % 3]) if k % 3 else (Q.FIXED, k % NUM_FIXED, rots[0])
            vals.append(g.add_calculation(Q.ADD, col, g.add_constant(1000 + k)))
            k += 1
        r = vals[0]
        for v in vals[1:]:
            r = g.add_calculation(Q.MUL, r, v)
        run = g.add_calculation(Q.HORNER, run, (Q.Y, 0, 0), [g.add_calculation(Q.SQUARE, r)])
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quotient", "probe.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("quotient_probe: no GPU")
    from tachyon_amd import params as P
    from tachyon_amd import plonk
    from tachyon_amd import plonk_quotient as Q

    r = P.FIELDS[FIELD][0]

    def mont(x):
        return P.mont(x, r, 4).to_bytes(32, "little")

    gen = torch.Generator(device="cuda").manual_seed(53)

    def poly(n):  # canonical Montgomery bytes: 253 random bits per element
        t = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen)
        t[:, 31] &= 0x1F
        return t.reshape(-1)

    S = Q.fast_slots()
    scalars = dict(theta=mont(0x7E7A), beta=mont(0xBE7A), gamma=mont(0x6A33A), y=mont(0x1234567))
    lookup = Q.GraphEvaluator.for_lookup([("advice", 0, 0), ("advice", 1, 1)], [("fixed", 0, 0), ("fixed", 1, 0)], FIELD)
    perm_columns = [("advice", i) for i in range(PERM_COLUMNS)]
    num_z = (PERM_COLUMNS + CS_DEGREE - 3) // (CS_DEGREE - 2)
    result = {"field": FIELD, "cs_degree": CS_DEGREE, "parts": 4, "tile_rows": Q.tile_rows(), "fast_slots": S,
              "columns": {"fixed": NUM_FIXED, "advice": NUM_ADVICE, "instance": NUM_INSTANCE},
              "permutation_columns": PERM_COLUMNS, "lookups": 1, "gate_blocks": args.blocks,
              "mulmod_ceiling_per_s": MULMOD_PER_S, "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps, "shapes": []}
    for log_n in args.log_n:
        n = 1 << log_n
        fixed = [poly(n) for _ in range(NUM_FIXED)]
        advice = [poly(n) for _ in range(NUM_ADVICE)]
        instance = [poly(n) for _ in range(NUM_INSTANCE)]
        shared = dict(l_first=poly(n), l_last=poly(n), l_active_row=poly(n))
        sigmas = [poly(n) for _ in range(PERM_COLUMNS)]
        circuit = dict(fixed=fixed, advice=advice, instance=instance, challenges=[],
                       perm_z=[poly(n) for _ in range(num_z)], lookups=[(poly(n), poly(n), poly(n))], shuffle_z=[])
        out = torch.zeros(32 * n * (CS_DEGREE - 1), dtype=torch.uint8, device="cuda")
        table = dict(fixed=fixed, advice=advice, instance=instance, cs_degree=CS_DEGREE, **scalars, **shared)
        for label, live in (("lds", S - 2), ("spill", 2 * S)):
            gates = gate_graph(Q, live, args.blocks)
            stats = {
                "gates": Q.quotient_program_stats(FIELD, n, Q.GATES, graph=gates, **table),
                "permutation": Q.quotient_program_stats(FIELD, n, Q.PERMUTATION, z=circuit["perm_z"], sigmas=sigmas,
                                                        perm_columns=perm_columns, x_scale=mont(3), omega=mont(5),
                                                        delta=plonk.get_delta(FIELD), **table),
                "lookups": Q.quotient_program_stats(FIELD, n, Q.LOOKUP, graph=lookup, z=[circuit["lookups"][0][0]],
                                                    a_perm=circuit["lookups"][0][1], s_perm=circuit["lookups"][0][2],
                                                    **table),
            }
            kw = dict(cs_degree=CS_DEGREE, last_row=-6, zeta=Q.get_zeta(FIELD), delta=plonk.get_delta(FIELD),
                      gates=gates, perm_columns=perm_columns, sigmas=sigmas, lookups=[lookup], **scalars, **shared)
            est = Q.quotient_work_bytes(FIELD, n, [circuit], **{k: v for k, v in kw.items() if k not in ("zeta", "delta")})
            samples, walls = [], []
            for _ in range(args.reps + 1):  # the first call loads the code objects: dropped
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert Q.quotient_h_poly(FIELD, n, [circuit], out=out, **kw) is out  # synchronises before it returns
                walls.append((time.perf_counter() - t0) * 1e3)
                samples.append(Q.last_timings())
            samples, walls = samples[1:], walls[1:]
            evaluator = lambda t: t["gates"] + t["permutation"] + t["lookups"] + t["shuffles"]
            best = min(samples, key=evaluator)
            rows = n * 4
            products = sum(s["products"] for s in stats.values())
            reads = sum(s["column_reads"] for s in stats.values())
            total = sum(best.values())
            entry = {"log_n": log_n, "variant": label, "gate_live_values": live, "programs": stats,
                     "products_per_row": products, "column_elements_per_row": reads, "ms": best, "samples": samples,
                     "ms_spans": total, "ms_evaluator": evaluator(best), "ms_wall": min(walls), "wall_samples": walls,
                     "evaluator_share_of_spans": evaluator(best) / total,
                     "transform_share_of_spans": (best["transforms"] + best["ifft"]) / total,
                     "evaluator_share_of_wall": evaluator(best) / min(walls),
                     "products_per_s": products * rows / (evaluator(best) * 1e-3),
                     "gate_products_per_s": stats["gates"]["products"] * rows / (best["gates"] * 1e-3),
                     "column_bytes_per_s": 32 * reads * rows / (evaluator(best) * 1e-3),
                     "work_bytes": est, "held_bytes": Q.held_bytes()}
            entry["mulmod_frac"] = entry["products_per_s"] / MULMOD_PER_S
            entry["gate_mulmod_frac"] = entry["gate_products_per_s"] / MULMOD_PER_S
            entry["hbm_frac"] = entry["column_bytes_per_s"] / HBM_BYTES_PER_S
            result["shapes"].append(entry)
        pair = result["shapes"][-2:]
        per_product = [e["ms"]["gates"] / e["programs"]["gates"]["products"] for e in pair]
        result.setdefault("spill_slowdown_per_gate_product", {})[str(log_n)] = per_product[1] / per_product[0]
        del fixed, advice, instance, shared, sigmas, circuit, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
