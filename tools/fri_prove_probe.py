#!/usr/bin/env python3
"""The opening proof in one call against the step-by-step API, at fri_probe.py's
shape (2^20 x 100 trace, log_blowup 1, 2 points, Horizen, device-resident, 100
queries, 16 proof-of-work bits), in one process, the legs alternating:

  (a) step_api   begin / add_round / commit / fold driven by a Python host
                 challenger (tests/fri_ref.DuplexChallenger), then 100 x
                 answer_query and 100 x open on the round tree: the path without
                 the library's challenger.  Its grind runs on the host
                 (fri_ref.grind) and is timed once, apart.
  (b) prove      FriOpening.prove with the library's DuplexChallenger, at 16
                 bits and at 0 bits (the same work as (a) without its grind)
  (c) grind      DuplexChallenger.grind alone at 16, 20 and 24 bits from a fixed
                 transcript: seconds, launches (from the chunk rule of
                 fri/grind_bb.h) and candidates scanned per second against
                 permute_kernel's states per second in the same run
  (d) gathers    answer_queries and open_batch at 100 indices against their
                 per-index loops

(a) and (b) must produce the same roots, final value and query indices when (a)
is given (b)'s witness: that is checked before anything is timed.  Every figure
is the best of `--reps` runs between device events (the calls wait inside), all
samples recorded.  Writes profiles/fri/prove_probe.json and prints the same JSON
line; fails without a GPU.

    python tools/fri_prove_probe.py [-k 20] [-b 100] [--reps 5] [--out profiles/fri/prove_probe.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIRST_CHUNK_MIN, CHUNK_MAX = 1 << 16, 1 << 24      # fri/grind_bb.h


def grind_chunks(bits: int, witness: int):
    """(launches, candidates scanned) of a grind over [0, p) that found `witness`"""
    first = min(max(4 << bits, FIRST_CHUNK_MIN), CHUNK_MAX)
    if witness < first:
        return 1, first
    later = (witness - first) // CHUNK_MAX + 1
    return 1 + later, first + later * CHUNK_MAX


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", type=int, default=20)
    ap.add_argument("-b", type=int, default=100)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--bits", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri", "prove_probe.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fri_prove_probe: no GPU")
    import fri_ref as F
    import poseidon2_ref as R
    from tachyon_amd import params
    from tachyon_amd.fri import DuplexChallenger, FriOpening
    from tachyon_amd.ntt import IcicleNTT, IcicleNTTOptions
    from tachyon_amd.poseidon2 import FieldMerkleTree, Poseidon2BabyBear

    p, cols, shift, log_blowup, external = params.BABY_BEAR, args.b, 31, 1, "horizen"
    rows = 1 << args.k
    n = rows << log_blowup
    log_max = args.k + log_blowup
    gen = params.baby_bear_mont(params.baby_bear_root_of_unity(n)).to_bytes(4, "little")
    ntt = IcicleNTT("baby_bear")
    assert ntt.init(gen, IcicleNTTOptions(are_inputs_on_device=1, are_outputs_on_device=1, is_async=1))
    stream_handle = ntt.stream
    stream = torch.cuda.ExternalStream(stream_handle)
    tree = FieldMerkleTree(external, stream_handle)
    fri = FriOpening(log_blowup, external, stream_handle)

    x = torch.randint(0, p, (rows * cols,), dtype=torch.int32, device="cuda")
    lde = torch.empty(n * cols, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert ntt.coset_lde_batch_ptr(x.data_ptr(), rows, cols, log_blowup, shift, lde.data_ptr())
    assert tree.build_ptr([(lde.data_ptr(), n, cols)], bit_reversed=True)
    root = tree.root

    def canon(data):
        return R.from_mont_words(R.from_bytes(data))

    # the transcript up to the opening points, in both challengers
    lib_start, ref_start = DuplexChallenger(external, 8), F.DuplexChallenger(external)
    assert lib_start.observe(root)
    ref_start.observe(canon(root))
    points = [lib_start.sample_ext(), lib_start.sample_ext()]
    assert [F.to_bytes(ref_start.sample_ext()) for _ in range(2)] == points
    mats = [(lde.data_ptr(), n, cols)]

    def step_api(witness=None):
        """(a) without its grind; the witness is handed in (any 16-bit witness
        costs the same here).  Returns what the proof consists of."""
        ch = ref_start.clone()
        if not fri.begin(F.to_bytes(ch.sample_ext())) or fri.add_round_ptr(mats, [points]) is None:
            return None

        def on_commit(r):
            ch.observe(canon(r))
            return F.to_bytes(ch.sample_ext())

        roots = fri.commit_phase(on_commit)
        final_eval = fri.final_eval
        ch.observe(F.from_bytes(final_eval)[0])
        if witness is not None:
            assert ch.check_witness(args.bits, witness)
        indices = [ch.sample_bits(log_max) for _ in range(args.queries)]
        steps = [fri.answer_query(i) for i in indices]
        inputs = [tree.open(i) for i in indices]
        return roots, final_eval, indices, steps, inputs

    def prove(bits):
        ch = lib_start.clone()
        got = fri.prove(ch, [(tree, [points])], args.queries, bits)
        ch.close()
        return got

    def timed(call):
        samples = []
        for rep in range(args.reps + 1):
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert call() is not None
            e1.record(stream)
            e1.synchronize()
            if rep:
                samples.append(e0.elapsed_time(e1) / 1e3)
        return {"seconds": min(samples), "samples": samples}

    out = {"probe": "fri_prove_baby_bear", "device": torch.cuda.get_device_name(0), "external": external,
           "log_rows": args.k, "cols": cols, "log_blowup": log_blowup, "points": 2, "queries": args.queries,
           "bits": args.bits, "reps": args.reps, "checks": {}}

    # ---- check: both paths make the same proof
    proof, _ = prove(args.bits)
    witness = int(R.from_mont_words([proof.pow_witness])[0])
    roots, final_eval, indices, steps, inputs = step_api(witness)
    out["checks"]["commits_equal"] = proof.commit_phase_commits == roots and len(roots) == args.k
    out["checks"]["final_eval_equal"] = proof.final_eval == final_eval
    out["checks"]["indices_equal"] = [proof.query_index(q) for q in range(args.queries)] == indices
    out["checks"]["openings_equal"] = all(proof.query_steps(q) == steps[q] and proof.query_input(q, 0) == inputs[q]
                                          for q in range(0, args.queries, 7))
    proof.close()
    if not all(out["checks"].values()):
        print(json.dumps(out))
        raise SystemExit("fri_prove_probe: a check failed")

    # ---- (a) against (b), alternating
    legs = {"step_api_without_grind": lambda: step_api(witness), "prove": lambda: prove(args.bits),
            "prove_0_bits": lambda: prove(0)}
    samples = {k: [] for k in legs}
    for rep in range(args.reps + 1):
        for name, call in legs.items():
            r = timed_once(stream, torch, call)
            if rep:
                samples[name].append(r)
    for name in legs:
        out[name] = {"seconds": min(samples[name]), "samples": samples[name]}
    ch = ref_start.clone()
    ch.sample_ext()
    for r in roots:
        ch.observe(canon(r))
        ch.sample_ext()
    ch.observe(F.from_bytes(final_eval)[0])
    t0 = time.perf_counter()
    host_witness = ch.grind(args.bits)
    out["host_grind"] = {"seconds": time.perf_counter() - t0, "samples": 1, "witness_equal": host_witness == witness}
    out["step_api"] = {"seconds": out["step_api_without_grind"]["seconds"] + out["host_grind"]["seconds"]}
    out["waits"] = {"step_api": 1 + args.k + 1 + 2 * args.queries, "prove": 1 + args.k + 1 + 1 + 1 + 1}

    # ---- (c) the grind alone
    count = 1 << 24
    states = torch.randint(0, p, (count * 16,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    perm = Poseidon2BabyBear(external)
    t = timed(lambda: perm.permute_ptr(states.data_ptr(), count, stream_handle) or None)
    out["permute_states_per_second"] = count / t["seconds"]
    del states
    out["grind"] = {}
    for bits in (16, 20, 24):
        fixed = DuplexChallenger(external, 8)
        assert fixed.observe(b"".join(v.to_bytes(4, "little") for v in range(1, 12)))      # raw words 1..11
        found = []

        def one():
            c = fixed.clone()
            w = c.grind(bits, stream_handle)
            c.close()
            found.append(w)
            return w

        t = timed(one)
        w = int(R.from_mont_words([found[0]])[0])
        launches, scanned = grind_chunks(bits, w)
        t.update({"witness": w, "launches": launches, "waits": launches, "candidates_scanned": scanned,
                  "candidates_per_second": scanned / t["seconds"],
                  "share_of_permute_rate": scanned / t["seconds"] / out["permute_states_per_second"]})
        out["grind"][str(bits)] = t
        fixed.close()

    # ---- (d) the gathers (the opening is in its ended state after the last prove)
    spread = [(q * 2654435761) % n for q in range(args.queries)]
    out["answer_queries"] = timed(lambda: fri.answer_queries(spread))
    out["answer_query_loop"] = timed(lambda: [fri.answer_query(i) for i in spread])
    out["open_batch"] = timed(lambda: tree.open_batch(spread))
    out["open_loop"] = timed(lambda: [tree.open(i) for i in spread])
    for k in ("answer_queries", "open_batch"):
        out[k].update({"launches": 1, "waits": 1})
    for k in ("answer_query_loop", "open_loop"):     # a batch of one per index
        out[k].update({"launches": args.queries, "waits": args.queries})

    fri.close()
    tree.close()
    ntt.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


def timed_once(stream, torch, call):
    """seconds of one call between device events on `stream`"""
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    assert call() is not None
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3


if __name__ == "__main__":
    main()
