#!/usr/bin/env python3
"""KZG opening probe over BN254, device-resident polynomials, at a halo2-like
shape: 64 polynomials of 2^20 coefficients opened at 3 points (x for all,
w x for the last 16, x / w for the last 4), under SHPlonk and under GWC.

Per scheme it records the phases of tachyon_mi355x_kzg_create_opening_proof --
combine (linear combinations), divide (divisions by linear factors), commit
(the MSMs) -- and, once, the batched evaluation that produces the claimed
values: milliseconds from stream events (the library's own, around each
phase), best of `--reps` with every sample kept.  For the three new kernel
families it adds the bytes they must move (every input read once and the
output written once; a division reads its input and writes its quotient once
per root) over the time, as a share of the HBM rate.

Beside them, the same proof done the only way the parent commit allows:
polynomials copied to the host, the quotients built there (linear
combinations through the oracle's C field operations, divisions as Python
integer recurrences, as tests/kzg_open_ref.py does them), uploaded again and
committed with commit_batch.  The two ways must give the same commitments.

Writes profiles/kzg_open/probe.json and prints the same JSON line; fails
without a GPU.

    python tools/kzg_open_probe.py [-k 20] [--polys 64] [--reps 3] [--no-baseline]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12
FIELD = "bn254_fr"


class Transcript:
    """Deterministic challenges; a written point is folded into the state."""

    def __init__(self, r):
        self.r, self.state, self.written = r, 0x5EED, []

    def squeeze(self):
        self.state = self.state * 2 % self.r
        return self.state

    def write(self, point):
        self.written.append(bytes(point))
        self.state = (self.state + int.from_bytes(bytes(point)[:31], "little")) % self.r
        return True


class LibTranscript(Transcript):
    def __init__(self, F):
        super().__init__(F.p)
        self.F = F

    def squeeze_challenge(self):
        return self.F.to_bytes(self.squeeze())

    def write_to_proof(self, point):
        return self.write(point)


def ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def raw(xs):
    return b"".join(x.to_bytes(32, "little") for x in xs)


class HostPolys:
    """The CPU side of the baseline: polynomials as Montgomery bytes; a linear
    combination is one product and one sum per input through the oracle's
    field operations, a division the reference's integer recurrence (linear,
    so it runs on the Montgomery integers as they are)."""

    def __init__(self, F):
        from oracle import oracle as O
        self.O, self.F = O, F

    def lincomb(self, polys, coeffs, d=0):
        n = max(len(p) for p in polys)
        acc = bytes(n)
        for p, c in zip(polys, coeffs):
            if not p:
                continue
            term = self.O.field_op(FIELD, "mul", p, self.F.to_bytes(c) * (len(p) // 32))
            acc = self.O.field_op(FIELD, "add", acc, term + bytes(n - len(term)))
        if d and n:
            acc = self.O.field_op(FIELD, "sub", acc[:32], self.F.to_bytes(d)) + acc[32:]
        return acc

    def divide(self, p, roots):
        import kzg_open_ref as R
        return raw(R.divide_by_roots(ints(p), roots, self.F.p)[0])


def host_prove(H, scheme, polys, openings, t):
    """The quotient polynomials of kzg_open_ref's provers, with the bulk
    arithmetic through HostPolys; returns them in the order they are committed
    (a generator: the transcript needs each commitment before going on)."""
    import kzg_open_ref as R
    r = H.F.p
    if scheme == "gwc":
        v = t.squeeze()
        for pts, idx, vals in R.group_by_single_point(openings):
            cs = [pow(v, j, r) for j in range(len(idx))]
            d = sum(c * val[0] for c, val in zip(cs, vals)) % r
            yield H.divide(H.lincomb([polys[i] for i in idx], cs, d), pts)
        return
    groups, sup = R.group_by_poly_and_points(openings), R.super_points(openings)
    y = t.squeeze()
    interp, hs = [], []
    for pts, idx, vals in groups:
        rs = [R.lagrange_interpolate(pts, val, r) for val in vals]
        interp.append(rs)
        cs = [pow(y, j, r) for j in range(len(idx))]
        rc = R.linear_combination(rs, cs, 0, r)
        num = H.lincomb([polys[i] for i in idx] + [b"".join(H.F.to_bytes(c) for c in rc)], cs + [r - 1])
        hs.append(H.divide(num, pts))
    v = t.squeeze()
    h = H.lincomb(hs, [pow(v, g, r) for g in range(len(groups))])
    yield h
    u = t.squeeze()
    zd = [R.vanishing_at([x for x in sup if x not in pts], u, r) for pts, _, _ in groups]
    inv = pow(zd[0], -1, r)
    terms, cs, d = [], [], 0
    for g, (pts, idx, vals) in enumerate(groups):
        for j, i in enumerate(idx):
            c = pow(v, g, r) * zd[g] * inv * pow(y, j, r) % r
            terms.append(polys[i])
            cs.append(c)
            d = (d + c * R.evaluate(interp[g][j], u, r)) % r
    yield H.divide(H.lincomb(terms + [h], cs + [-R.vanishing_at(sup, u, r) * inv % r], d), [u])


def must_move_bytes(scheme, n, group_sizes, group_points):
    """(combine, divide) bytes for polynomials of n coefficients."""
    e = 32 * n
    if scheme == "gwc":
        return sum((c + 1) * e for c in group_sizes), 2 * e * len(group_sizes)
    combine = sum((c + 1) * e for c in group_sizes) + (len(group_sizes) + 1) * e + (sum(group_sizes) + 2) * e
    return combine, 2 * e * (sum(group_points) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", type=int, default=20)
    ap.add_argument("--polys", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_open", "probe.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("kzg_open_probe: no GPU")
    import kzg_open_ref as R
    from oracle import pyref
    from tachyon_amd.kzg import KZG

    F = pyref.Field(FIELD)
    n, m = 1 << args.k, args.polys
    gen = torch.Generator(device="cuda").manual_seed(20)
    polys = []
    for _ in range(m):  # canonical Montgomery bytes: 253 random bits per element
        t = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen)
        t[:, 31] &= 0x1F
        polys.append(t.reshape(-1))
    torch.cuda.synchronize()
    kzg = KZG("bn254_g1")
    t0 = time.perf_counter()
    kzg.unsafe_setup(n, F.to_bytes(0x1234567890ABCDEF))
    setup_s = time.perf_counter() - t0

    x = 0x0123456789ABCDEF0123456789ABCDEF % F.p
    w = F.root_of_unity(n)
    pairs = [(i, x) for i in range(m)] + [(i, x * w % F.p) for i in range(m - m // 4, m)]
    pairs += [(i, x * pow(w, -1, F.p) % F.p) for i in range(m - m // 16, m)]
    lib_pairs = [(i, F.to_bytes(z)) for i, z in pairs]

    result = {"shape": {"curve": "bn254_g1", "log_n": args.k, "polys": m, "points": 3, "openings": len(pairs)},
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "setup_s": round(setup_s, 3), "reps": args.reps}

    # the claimed values: one batched evaluation (warm-up, then timed)
    values = kzg.evaluate(polys, lib_pairs)
    ev = []
    for _ in range(args.reps):
        assert kzg.evaluate(polys, lib_pairs) == values
        ev.append(kzg.last_open_timings()["evaluate"])
    ev_bytes = 32 * n * len(pairs)
    result["evaluate"] = {"ms": min(ev), "samples_ms": ev, "bytes": ev_bytes,
                          "hbm_share": ev_bytes / (min(ev) * 1e-3) / HBM_BYTES_PER_S}
    print(f"[kzg_open_probe] evaluate: {min(ev):.3f} ms", file=sys.stderr, flush=True)
    openings = [(i, z, F.from_bytes(v)) for (i, z), v in zip(pairs, values)]
    lib_open = [(i, F.to_bytes(z), v) for (i, z), v in zip(pairs, values)]

    host = None
    for scheme in ("shplonk", "gwc"):
        groups = R.group_by_single_point(openings) if scheme == "gwc" else R.group_by_poly_and_points(openings)
        cb, db = must_move_bytes(scheme, n, [len(g[1]) for g in groups], [len(g[0]) for g in groups])
        proof = kzg.create_opening_proof(polys, lib_open, LibTranscript(F), scheme=scheme)  # warm-up
        assert proof is not None
        samples, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            assert kzg.create_opening_proof(polys, lib_open, LibTranscript(F), scheme=scheme) == proof
            wall.append((time.perf_counter() - t0) * 1e3)
            samples.append(kzg.last_open_timings())
        best = {ph: min(s[ph] for s in samples) for ph in ("combine", "divide", "commit")}
        rec = {"groups": [[len(g[0]), len(g[1])] for g in groups], "ms": best, "samples_ms": samples,
               "call_ms": min(wall), "call_samples_ms": wall,
               "combine_bytes": cb, "combine_hbm_share": cb / (best["combine"] * 1e-3) / HBM_BYTES_PER_S,
               "divide_bytes": db, "divide_hbm_share": db / (best["divide"] * 1e-3) / HBM_BYTES_PER_S}
        if not args.no_baseline:
            # the parent commit's way: to the host, quotients on the CPU, back, commit_batch
            H = HostPolys(F)
            t0 = time.perf_counter()
            if host is None:
                host = [p.cpu().numpy().tobytes() for p in polys]
            to_host_s = time.perf_counter() - t0
            t = Transcript(F.p)
            cpu_s = commit_s = 0.0
            t0 = time.perf_counter()
            pending = []
            for q in host_prove(H, scheme, host, openings, t):
                cpu_s += time.perf_counter() - t0
                if scheme == "gwc":
                    pending.append(q)  # one commit_batch for every W, as the reference does
                else:
                    t1 = time.perf_counter()
                    t.write(kzg.commit_batch([q])[0])
                    commit_s += time.perf_counter() - t1
                t0 = time.perf_counter()
            if pending:
                t1 = time.perf_counter()
                for c in kzg.commit_batch(pending):
                    t.write(c)
                commit_s += time.perf_counter() - t1
            assert t.written == proof, "the host way and the device way disagree"
            rec["parent_commit_way_ms"] = {"to_host": to_host_s * 1e3, "cpu_quotients": cpu_s * 1e3,
                                           "upload_and_commit": commit_s * 1e3,
                                           "total": (to_host_s + cpu_s + commit_s) * 1e3,
                                           "note": "to_host is paid once (first scheme measured)"}
        result[scheme] = rec
        print(f"[kzg_open_probe] {scheme}: {json.dumps(rec['ms'])}", file=sys.stderr, flush=True)
    kzg.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
