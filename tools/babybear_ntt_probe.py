#!/usr/bin/env python3
"""BabyBear NTT probe: device-resident FFTBatch and CosetLDEBatch
(added_bits = 1, shift 31) at the shapes of the reference's benchmark/fft_batch
(-k 20..24, -b 100), and the consecutive layout at 2^20 and 2^24 with batch 1.

Outputs are first compared across layouts (a column of the matrix result
against the consecutive transform of that column); then each call is warmed up
and timed with device events over windows of >= 0.3 s.  Per shape the JSON
carries the launches per call, the bytes its passes move (from the shapes: every
pass reads and writes its matrix once), that figure over 8 TB/s as the HBM
share of the measured time, and the host-resident time (the reference times
host data).  Prints one JSON line; fails without a GPU.

    python tools/babybear_ntt_probe.py [-k 20 21 22 23 24] [-b 100] [--host-max-k 22]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
WINDOW_S = 0.3
MAX_PASS_STAGES = 10  # ntt_bb.h: BbGenDomain::kMaxPassStages


def passes(log_n: int) -> int:
    return (log_n + MAX_PASS_STAGES - 1) // MAX_PASS_STAGES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", type=int, nargs="+", default=[20, 21, 22, 23, 24])
    ap.add_argument("-b", type=int, default=100)
    ap.add_argument("--consecutive-k", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--host-max-k", type=int, default=22, help="host-resident timing up to this k")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("babybear_ntt_probe: no GPU")
    from tachyon_amd import params
    from tachyon_amd.ntt import IcicleNTT, IcicleNTTOptions

    p, cols, shift = params.BABY_BEAR, args.b, 31
    log_order = max(max(args.k) + 1, max(args.consecutive_k))
    gen = params.baby_bear_mont(params.baby_bear_root_of_unity(1 << log_order)).to_bytes(4, "little")
    dev = IcicleNTT("baby_bear")
    assert dev.init(gen, IcicleNTTOptions(are_inputs_on_device=1, are_outputs_on_device=1, is_async=1))
    host = IcicleNTT("baby_bear")
    assert host.init(gen)
    stream = torch.cuda.ExternalStream(dev.stream)

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

    def host_timed(call):
        call()
        t0 = time.perf_counter()
        call()
        return time.perf_counter() - t0

    def report(seconds, reps, launches, moved):
        return {"seconds": seconds, "calls_per_window": reps, "launches_per_call": launches, "bytes_moved": moved,
                "hbm_share_of_8TBps": moved / HBM_BYTES_PER_S / seconds}

    out = {"probe": "babybear_ntt", "device": torch.cuda.get_device_name(0), "cols": cols, "shift": shift,
           "added_bits": 1, "fft_batch": {}, "coset_lde_batch": {}, "consecutive": {}, "checks": {}}

    for k in args.k:
        rows = 1 << k
        words = rows * cols
        x = rand_words(words)
        mat = x.clone()
        lde = torch.empty(2 * words, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        # ---- agreement across layouts, column 0 and the last column
        assert dev.run_matrix_ptr(mat.data_ptr(), rows, cols)
        assert dev.coset_lde_batch_ptr(x.data_ptr(), rows, cols, 1, shift, lde.data_ptr())
        sync()
        ok = True
        for c in (0, cols - 1):
            col = x.view(rows, cols)[:, c].contiguous()
            one = col.clone()
            torch.cuda.synchronize()
            assert dev.run_ptr(one.data_ptr(), rows)
            sync()
            ok = ok and bool(torch.equal(one, mat.view(rows, cols)[:, c]))
            # the extension through the consecutive layout: inverse, zero padding, forward on the coset
            ext = torch.zeros(2 * rows, dtype=torch.int32, device="cuda")
            ext[:rows] = col
            torch.cuda.synchronize()
            assert dev.run_ptr(ext.data_ptr(), rows, inverse=True)
            assert dev.run_ptr(ext.data_ptr(), 2 * rows, coset=shift)
            sync()
            ok = ok and bool(torch.equal(ext, lde.view(2 * rows, cols)[:, c]))
        # FFTBatch then its inverse gives the input back
        assert dev.run_matrix_ptr(mat.data_ptr(), rows, cols, inverse=True)
        sync()
        ok = ok and bool(torch.equal(mat, x))
        out["checks"][str(k)] = ok
        if not ok:
            print(json.dumps(out))
            raise SystemExit(f"babybear_ntt_probe: layouts disagree at k={k}")

        # ---- timing, device-resident
        s, reps = timed(lambda: dev.run_matrix_ptr(mat.data_ptr(), rows, cols))
        fft = report(s, reps, dev.last_launches, passes(k) * 2 * words * 4)
        s, reps = timed(lambda: dev.coset_lde_batch_ptr(x.data_ptr(), rows, cols, 1, shift, lde.data_ptr()))
        moved = (passes(k) * 2 * words + (words + 2 * words) + (passes(k + 1) - 1) * 2 * 2 * words) * 4
        ldr = report(s, reps, dev.last_launches, moved)
        del mat, lde
        # ---- host-resident (copies in and out included)
        if k <= args.host_max_k:
            hx = x.cpu().numpy().tobytes()
            import ctypes
            src = ctypes.create_string_buffer(hx, len(hx))
            dst = ctypes.create_string_buffer(2 * len(hx))
            fft["host_resident_seconds"] = host_timed(lambda: host.run_matrix_ptr(ctypes.addressof(src), rows, cols))
            ldr["host_resident_seconds"] = host_timed(
                lambda: host.coset_lde_batch_ptr(ctypes.addressof(src), rows, cols, 1, shift, ctypes.addressof(dst)))
            del src, dst, hx
        out["fft_batch"][str(k)] = fft
        out["coset_lde_batch"][str(k)] = ldr
        del x
        torch.cuda.empty_cache()

    for k in args.consecutive_k:
        n = 1 << k
        x = rand_words(n)
        s, reps = timed(lambda: dev.run_ptr(x.data_ptr(), n))
        out["consecutive"][str(k)] = report(s, reps, dev.last_launches, passes(k) * 2 * n * 4)
        del x

    out["table_bytes"] = dev.table_bytes
    dev.close()
    host.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
