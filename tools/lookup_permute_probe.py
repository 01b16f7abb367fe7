#!/usr/bin/env python3
"""Permuted lookup columns probe over BN254 Fr, everything device-resident:
one pair and four pairs at n = 2^20 and 2^22 rows, A' and S' written into CUDA
tensors.  Two contents: a duplicate-free random table with every input row
holding the value of a random usable table row (about 37 % of the rows repeat),
and the all-equal input (every row the value of one table row: one first row,
u - 1 repeated rows, the leftover is the whole table but one).

Per shape it records the four phases of tachyon_mi355x_lookup_permute_pairs
(sort, search, ranks, write) in milliseconds from the library's own stream
events (tachyon_mi355x_lookup_permute_last_timings), best of `--reps` with
every sample kept, the whole call on the host clock, and beside them the bytes
each phase must move (the formulas are in DESIGN 4.10; the search's probes,
mostly cache hits, are counted apart as an upper bound).  From the same run:
the sort phase of tachyon_mi355x_log_lookup_m_polys over two lookups, which is
two bare FrSort runs of u elements and nothing else (the floor the design
accepts), and KZG.commit_lagrange of one column at the same size (the
neighbour: both columns are committed next), so that the step's share of
"permute and commit both columns" can be read off.

Writes profiles/lookup_permute/probe.json and prints the same JSON line; fails
without a GPU.

    python tools/lookup_permute_probe.py [--log-n 20 22] [--pairs 1 4] [--reps 5] [--no-commit]
"""
import argparse
import json
import math
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
FIELD = "bn254_fr"


def probe_bytes_at_most(u):
    """The search's probes of one pair were every row a first row and every probe a miss in the caches:
    log2(u) probes of a 16-byte key half each."""
    return u * math.ceil(math.log2(u)) * 16


def must_move(n, u, block):
    """Bytes each phase cannot avoid for one pair: what it reads once and writes once."""
    e, tiles = 32, -(-u // block)
    return {"sort": 2 * (e * u + e * u + 4 * u),  # per column: the elements in; the sorted keys and the permutation out
            # the keys of A in (the neighbour comes from the same lines), the two flags out (and consumed zeroed
            # before); the probes are counted apart: they are served mostly by the caches
            "search": e * u + 3 * u,
            # count: both flags in; carry: the tile counts in and out; compact: a flag in, leftpos out
            "ranks": 2 * u + 4 * 2 * 2 * tiles + u + 4 * u,
            # a flag, both permutations, leftpos and an element of A and of S in (a 32-byte element through a
            # permutation costs a whole 64-byte line at least), A' and S' out over n rows, the blinds in
            "write": u + 3 * 4 * u + 2 * 64 * u + 2 * e * n + 2 * e * (n - u)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-commit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_permute", "probe.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lookup_permute_probe: no GPU")
    from tachyon_amd import log_lookup as LL
    from tachyon_amd import lookup_permute as LP
    from tachyon_amd import params as P
    from tachyon_amd.kzg import KZG

    r = P.FIELDS[FIELD][0]

    def mont(x):
        return P.mont(x, r, 4).to_bytes(32, "little")

    gen = torch.Generator(device="cuda").manual_seed(50)

    def column(n):  # canonical Montgomery bytes: 253 random bits per element
        t = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen)
        t[:, 31] &= 0x1F
        return t

    header = open(os.path.join(ROOT, "tachyon_amd", "csrc", "plonk", "lookup_permute.h")).read()
    block = int(re.search(r"constexpr unsigned kLpBlock = (\d+);", header).group(1))
    result = {"field": FIELD, "block_rows": block, "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps, "shapes": []}
    most = max(args.pairs)
    for log_n in args.log_n:
        n = 1 << log_n
        u = n - 6
        tables = [column(n) for _ in range(most)]
        drawn = [t[torch.randint(0, u, (n,), device="cuda", generator=gen)].reshape(-1) for t in tables]
        equal = [t[17].repeat(n) for t in tables]  # every row the value of table row 17
        tables = [t.reshape(-1) for t in tables]
        outs = [(torch.empty(32 * n, dtype=torch.uint8, device="cuda"),
                 torch.empty(32 * n, dtype=torch.uint8, device="cuda")) for _ in range(most)]
        blinds = b"".join(mont(1000 + j) for j in range(2 * (n - u)))
        torch.cuda.synchronize()

        def timed(call, phases, timings):
            first = call()  # warm-up
            assert first is not None
            samples, wall = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                again = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                assert again[-1] == first[-1]
                ms = timings()
                samples.append({ph: ms[ph] for ph in phases})
            return first, {ph: min(s[ph] for s in samples) for ph in phases}, samples, wall

        # two bare FrSort runs of u elements: the sort phase of m_polys over two lookups
        two = [([drawn[0]], tables[0]), ([drawn[0]], drawn[0])]
        m_out = [torch.empty(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
        _, sort_best, sort_samples, _ = timed(lambda: LL.m_polys(FIELD, n, u, two, out=m_out), ("sort",),
                                              LL.last_timings)
        del m_out
        for count in args.pairs:
            rec = {"log_n": log_n, "usable_rows": u, "pairs": count, "must_move_bytes_per_pair": must_move(n, u, block),
                   "search_probe_bytes_per_pair_at_most": probe_bytes_at_most(u),
                   "two_bare_sorts_ms": sort_best["sort"], "two_bare_sorts_samples_ms": sort_samples}
            for name, inputs in (("drawn_from_a_duplicate_free_table", drawn), ("all_equal_inputs", equal)):
                pairs = list(zip(inputs[:count], tables[:count]))
                (_, _, misses), best, samples, wall = timed(
                    lambda: LP.permute_pairs(FIELD, n, u, pairs, blinds * count, out=outs[:count]), LP.PHASES,
                    LP.last_timings)
                assert misses == [0] * count
                moved = rec["must_move_bytes_per_pair"]
                rec[name] = {"ms": best, "phases_ms": sum(best.values()), "samples_ms": samples, "call_ms": min(wall),
                             "call_samples_ms": wall,
                             "after_sort_over_sort": (sum(best.values()) - best["sort"]) / best["sort"],
                             "hbm_share": {ph: count * moved[ph] / (best[ph] * 1e-3) / HBM_BYTES_PER_S for ph in best}}
                print(f"[lookup_permute_probe] 2^{log_n} x {count} {name}: {json.dumps(best)} call {min(wall):.3f}",
                      file=sys.stderr, flush=True)
            result["shapes"].append(rec)
        if not args.no_commit:
            kzg = KZG("bn254_g1")
            kzg.unsafe_setup(n, mont(0x1234567890ABCDEF))
            assert kzg.commit_lagrange(outs[0][0]) is not None  # warm-up
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                kzg.commit_lagrange(outs[0][0])
                ts.append((time.perf_counter() - t0) * 1e3)
            kzg.close()
            for rec in result["shapes"]:
                if rec["log_n"] == log_n:
                    rec["commit_lagrange_one_column_ms"] = min(ts)
                    rec["commit_lagrange_samples_ms"] = ts
                    # the pairs permuted, against the pairs permuted and both columns of each committed
                    made = rec["drawn_from_a_duplicate_free_table"]["call_ms"]
                    rec["share_of_permute_and_commit"] = made / (made + 2 * rec["pairs"] * min(ts))
        del tables, drawn, equal, outs

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
