#!/usr/bin/env python3
"""The drop-in IcicleNTT holder against plain domains of the same size
(NTT section): one process, BN254 Fr, a holder initialised at
2^--log-order, device-resident asynchronous forward transforms.

  python tools/icicle_ntt_probe.py --log-order 24 --log-m 24 20 --reps 50 --windows 6

Per size: the outputs of both paths are compared bytewise, both are warmed
up, then windows of --reps transforms alternate between the plain domain
(tachyon_mi355x_ntt_domain_transform_device) and the holder, each timed with
device events on its own stream; a second round swaps the two data buffers.
Also: init time and table bytes at the order, and at the last size the first
call with a new coset against the same call with cached tables.  Prints one
JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # BN254 Fr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-order", type=int, default=24)
    ap.add_argument("--log-m", type=int, nargs="+", default=[24, 20])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=6)
    args = ap.parse_args()
    import torch
    from tachyon_amd import msm as M
    from tachyon_amd.ntt import FieldEvaluationDomain, IcicleNTT, IcicleNTTOptions

    def window(fn, stream_ptr, reps):
        s = torch.cuda.ExternalStream(stream_ptr)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(reps):
            fn()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b) / reps

    out = {"field": "bn254_fr", "log_order": args.log_order, "reps": args.reps}
    # w_N = 5^((r - 1) / N) in Montgomery form (x 2^256 mod r)
    gen = (pow(5, (R - 1) >> args.log_order, R) << 256) % R
    h = IcicleNTT("bn254_fr")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if not h.init(gen.to_bytes(32, "little"),
                  IcicleNTTOptions(are_inputs_on_device=1, are_outputs_on_device=1, is_async=1)):
        raise SystemExit("init refused")
    out["init_ms"] = (time.perf_counter() - t0) * 1e3
    out["table_bytes"] = h.table_bytes

    n = 1 << max(args.log_m)
    base = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    M.gen_scalars("bn254_fr", 99, n, base.data_ptr())
    torch.cuda.synchronize()
    for log_m in args.log_m:
        m = 1 << log_m
        plain = FieldEvaluationDomain("bn254_fr", m)
        a, b = base[:m * 32].clone(), base[:m * 32].clone()
        torch.cuda.synchronize()
        sp, sh = torch.cuda.ExternalStream(plain.stream), torch.cuda.ExternalStream(h.stream)
        for inverse in (False, True):
            plain.transform_device(a.data_ptr(), 1, inverse)
            assert h.run_ptr(b.data_ptr(), m, inverse=inverse)
            sp.synchronize()
            sh.synchronize()
            assert torch.equal(a, b), (log_m, inverse)
        assert torch.equal(a, base[:m * 32])

        res = {"outputs_equal": True}
        # the data buffers swapped in the second round: a gap that follows the
        # buffer is placement, one that follows the path is the path's
        for rnd, (pa, pb) in enumerate(((a, b), (b, a))):
            def f_plain():
                plain.transform_device(pa.data_ptr(), 1, False)

            def f_holder():
                h.run_ptr(pb.data_ptr(), m)

            for _ in range(10):
                f_plain()
                f_holder()
            sp.synchronize()
            sh.synchronize()
            pw, hw = [], []
            for _ in range(args.windows):
                pw.append(round(window(f_plain, plain.stream, args.reps), 5))
                hw.append(round(window(f_holder, h.stream, args.reps), 5))
            res["plain_ms" if rnd == 0 else "plain_ms_swapped"] = pw
            res["holder_ms" if rnd == 0 else "holder_ms_swapped"] = hw
        out[f"2^{log_m}"] = res
        if log_m == args.log_m[-1]:
            first, cached = [], []
            for c in (11, 13, 17, 19, 23):
                first.append(round(window(lambda: h.run_ptr(b.data_ptr(), m, coset=c), h.stream, 1), 5))
                cached.append(round(window(lambda: h.run_ptr(b.data_ptr(), m, coset=c), h.stream, 1), 5))
            out[f"2^{log_m}"].update(new_coset_first_call_ms=first, cached_coset_call_ms=cached)
            out["table_bytes_with_5_cosets"] = h.table_bytes
        plain.close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
