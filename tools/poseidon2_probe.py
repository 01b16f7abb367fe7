#!/usr/bin/env python3
"""Poseidon2 / FieldMerkleTree probe over BabyBear, device-resident:

  permute      permutations per second of the batch kernel, and in the same run
               the in-register bb31::mul rate (tachyon_mi355x_baby_bear_mul_rate).
               A permutation is 564 Montgomery products (8 x 16 + 13 s-boxes of
               4), so permutations/s x 564 over the product rate is the share of
               the VALU roofline the kernel reaches; its additions and the
               internal layer's reductions come on top of the products.
  build        FieldMerkleTree builds of one 2^k x cols matrix, k = 18..21
  lde_commit   CosetLDEBatch (added_bits = 1, shift 31) followed by the
               bit-reversed build on the same stream, at 2^20 x cols

Results are first compared: the permutation of 0..15 against the reference's
known answer, and the bit-reversed build of a matrix against the plain build of
its row-permuted copy.  Each call is warmed up and timed with device events
over windows of >= 0.3 s.  Writes profiles/poseidon2/probe.json and prints the
same JSON line; fails without a GPU.

    python tools/poseidon2_probe.py [-k 18 19 20 21] [-b 100] [--lde-k 20] [--out profiles/poseidon2/probe.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
WINDOW_S = 0.3
PRODUCTS_PER_PERMUTATION = (8 * 16 + 13) * 4
KNOWN_ANSWER = [1699737005, 296394369, 268410240, 828329642, 1491697358, 1128780676, 287184043, 1806152977,
                1380147856, 345666717, 491196631, 1875224538, 697740550, 1854502887, 1201727753, 1802410886]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", type=int, nargs="+", default=[18, 19, 20, 21])
    ap.add_argument("-b", type=int, default=100)
    ap.add_argument("--lde-k", type=int, default=20)
    ap.add_argument("--permute-log-count", type=int, default=22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon2", "probe.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("poseidon2_probe: no GPU")
    from tachyon_amd import params
    from tachyon_amd.ntt import IcicleNTT, IcicleNTTOptions
    from tachyon_amd.poseidon2 import FieldMerkleTree, Poseidon2BabyBear, mul_rate

    p, cols, shift = params.BABY_BEAR, args.b, 31
    gen = params.baby_bear_mont(params.baby_bear_root_of_unity(1 << (args.lde_k + 1))).to_bytes(4, "little")
    ntt = IcicleNTT("baby_bear")
    assert ntt.init(gen, IcicleNTTOptions(are_inputs_on_device=1, are_outputs_on_device=1, is_async=1))
    stream_handle = ntt.stream
    stream = torch.cuda.ExternalStream(stream_handle)
    tree = FieldMerkleTree("horizen", stream_handle)
    perm = Poseidon2BabyBear("horizen")

    def sync():
        stream.synchronize()
        torch.cuda.synchronize()

    def rand_words(count):
        t = torch.randint(0, p, (count,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return t

    def timed(call):
        """seconds per call: warm up, then event-timed windows of >= 0.3 s"""
        assert call()
        sync()

        def window(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                assert call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / 1e3

        reps = 1
        while True:
            w = window(reps)
            if w >= WINDOW_S:
                return min(w, window(reps)) / reps, reps  # the better of two full windows
            reps = max(2 * reps, int(reps * WINDOW_S / max(w, 1e-6) * 1.2) + 1)

    out = {"probe": "poseidon2_baby_bear", "device": torch.cuda.get_device_name(0), "external": "horizen",
           "cols": cols, "checks": {}, "permute": {}, "build": {}, "lde_commit": {}}

    # ---- checks
    r_mod = params.BABY_BEAR_R % p
    r_inv = pow(params.BABY_BEAR_R, -1, p)
    kat = b"".join((i * r_mod % p).to_bytes(4, "little") for i in range(16))
    got = perm.permute(kat)
    out["checks"]["known_answer"] = got is not None and [
        int.from_bytes(got[4 * i:4 * i + 4], "little") * r_inv % p for i in range(16)] == KNOWN_ANSWER
    rows = 1 << 12
    x = rand_words(rows * cols)
    idx = torch.arange(rows, device="cuda")
    rev = torch.zeros_like(idx)
    for b in range(12):
        rev |= ((idx >> b) & 1) << (11 - b)
    permuted = x.view(rows, cols)[rev].contiguous()
    torch.cuda.synchronize()
    other = FieldMerkleTree("horizen", stream_handle)
    assert tree.build_ptr([(x.data_ptr(), rows, cols)], bit_reversed=True)
    assert other.build_ptr([(permuted.data_ptr(), rows, cols)])
    out["checks"]["bit_reversed_equals_permuted"] = tree.layers() == other.layers() and tree.root is not None
    other.close()
    del x, permuted
    if not all(out["checks"].values()):
        print(json.dumps(out))
        raise SystemExit("poseidon2_probe: a check failed")

    # ---- the permutation kernel and the product rate, in the same run
    count = 1 << args.permute_log_count
    states = rand_words(16 * count)
    s, reps = timed(lambda: perm.permute_ptr(states.data_ptr(), count, stream_handle))
    products = mul_rate(1 << 22, 4096)
    out["permute"] = {
        "states": count, "seconds": s, "calls_per_window": reps, "permutations_per_second": count / s,
        "products_per_permutation": PRODUCTS_PER_PERMUTATION,
        "bb31_mul_products_per_second": products,
        "valu_roofline_share": count / s * PRODUCTS_PER_PERMUTATION / products if products else None,
        "bytes_moved": 2 * 64 * count, "hbm_share_of_8TBps": 2 * 64 * count / HBM_BYTES_PER_S / s,
    }
    del states

    # ---- builds
    for k in args.k:
        rows = 1 << k
        x = rand_words(rows * cols)
        s, reps = timed(lambda: tree.build_ptr([(x.data_ptr(), rows, cols)]))
        permutations = rows * ((cols + 7) // 8) + rows - 1
        moved = rows * cols * 4 + 32 * (rows + 3 * (rows - 1))  # the matrix once; every layer written, read by the next
        out["build"][str(k)] = {
            "rows": rows, "seconds": s, "calls_per_window": reps, "launches_per_call": tree.last_launches,
            "permutations": permutations, "permutations_per_second": permutations / s,
            "bytes_moved": moved, "hbm_share_of_8TBps": moved / HBM_BYTES_PER_S / s,
        }
        del x
        torch.cuda.empty_cache()

    # ---- TwoAdicFRI::Commit: the extension, then the bit-reversed build, one stream, no wait in between
    k = args.lde_k
    rows = 1 << k
    x = rand_words(rows * cols)
    lde = torch.empty(2 * rows * cols, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def lde_only():
        return ntt.coset_lde_batch_ptr(x.data_ptr(), rows, cols, 1, shift, lde.data_ptr())

    def commit():
        return lde_only() and tree.build_ptr([(lde.data_ptr(), 2 * rows, cols)], bit_reversed=True)

    s_lde, _ = timed(lde_only)
    s_build, _ = timed(lambda: tree.build_ptr([(lde.data_ptr(), 2 * rows, cols)], bit_reversed=True))
    s, reps = timed(commit)
    out["lde_commit"] = {"log_rows": k, "added_bits": 1, "shift": shift, "seconds": s, "calls_per_window": reps,
                         "lde_seconds": s_lde, "bit_reversed_build_seconds": s_build,
                         "launches_lde": ntt.last_launches, "launches_build": tree.last_launches}

    tree.close()
    ntt.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
