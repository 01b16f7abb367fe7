"""GPU NTT parity through the C-ABI (the reference's
univariate_evaluation_domain_gpu_unittest.cc:20-66 and fft_benchmark_gpu.cc
--check_results): FFT/IFFT outputs bytewise equal to the CPU oracle, plain and
coset, plus size-independent properties at the benchmark sizes."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def domain(n):
    from tachyon_amd.ntt import Radix2EvaluationDomain
    return Radix2EvaluationDomain(n)


def test_ntt_golden():
    g = json.load(open(os.path.join(GOLDEN, "ntt_bn254_fr.json")))
    for c in g["cases"]:
        n = 1 << c["log_n"]
        d = domain(n)
        if c["offset"] != 1:
            d.set_offset(bytes.fromhex(c["offset_mont"]))
        coeffs = b"".join(bytes.fromhex(x) for x in c["coeffs"])
        ev = d.fft(coeffs)
        assert ev.hex() == "".join(c["evals"]), c
        assert d.ifft(ev).hex() == "".join(c["ifft_of_evals"]), c
        d.close()


@pytest.mark.parametrize("logn", list(range(5, 15)) + [16, 18, 20])
def test_fft_ifft_vs_oracle(logn):
    n = 1 << logn
    coeffs = O.gen_scalars("bn254_fr", 1000 + logn, n).tobytes()
    d = domain(n)
    ev = d.fft(coeffs)
    assert ev == O.fft(coeffs, n)
    assert d.ifft(ev) == O.ifft(ev, n)


@pytest.mark.parametrize("logn", [5, 9, 14])
def test_coset_vs_oracle(logn):
    """offset = subgroup generator 5 (univariate_evaluation_domain_gpu_unittest.cc:62-64)."""
    n = 1 << logn
    five = O.field_op("bn254_fr", "to_mont", (5).to_bytes(32, "little"))
    coeffs = O.gen_scalars("bn254_fr", 2000 + logn, n).tobytes()
    d = domain(n)
    d.set_offset(five)
    ev = d.fft(coeffs)
    assert ev == O.fft(coeffs, n, five)
    assert d.ifft(ev) == O.ifft(ev, n, five)


def test_degree_aware_and_empty():
    n = 1 << 10
    d = domain(n)
    for m in (1, 3, 100, 257, 1024):
        coeffs = O.gen_scalars("bn254_fr", m, m).tobytes()
        assert d.fft(coeffs) == O.fft(coeffs, n), m
    assert d.fft(b"") == b""       # FFT of the zero polynomial is empty Evals
    assert d.ifft(b"") == b""


def test_device_round_trip_2_24():
    """Config 3 at the north-star size: forward then inverse returns the input
    bytewise; FFT is linear (FFT(a+b) = FFT(a)+FFT(b) checked on a slice)."""
    torch = pytest.importorskip("torch")
    from tachyon_amd import msm as M
    logn = 24
    n = 1 << logn
    d = domain(n)
    x = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    M.gen_scalars("bn254_fr", 24, n, x.data_ptr())
    torch.cuda.synchronize()
    ref = x.clone()
    d.transform_device(x.data_ptr(), inverse=False)
    d.transform_device(x.data_ptr(), inverse=True)
    torch.cuda.synchronize()
    assert torch.equal(x, ref)
    # spot-check evaluations: e_i = sum_j c_j w^(ij) for a few i via the oracle's Horner is
    # too slow at 2^24; instead compare one full transform at 2^20 elsewhere and check
    # here that the forward transform of a delta is all-ones (c_0 = 1 -> e_i = 1).
    one = O.field_op("bn254_fr", "to_mont", (1).to_bytes(32, "little"))
    y = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    y[:32] = torch.frombuffer(bytearray(one), dtype=torch.uint8).cuda()
    d.transform_device(y.data_ptr(), inverse=False)
    torch.cuda.synchronize()
    ones = torch.frombuffer(bytearray(one * 1024), dtype=torch.uint8).cuda()
    assert torch.equal(y[:32 * 1024], ones) and torch.equal(y[-32 * 1024:], ones)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("log_n,world", [(2, 1), (6, 2), (9, 4), (12, 8), (13, 8), (20, 8), (14, 1), (19, 2)])
def test_four_step_simulated_ranks(log_n, world, variant):
    """The distributed four-step plan on one GPU with `world` simulated ranks:
    stage 1 on every rank, the all-to-all done by slicing, stage 2 -> each
    rank's slab of the oracle FFT; the inverse returns every rank's input.
    Every plan variant (the exchange's twiddle + packing fused into the
    sub-transforms' passes or the round-4 separate kernels; 29- or 32-bit
    passes) gives the same bytes."""
    _four_step_round_trip(log_n, world, variant)


@pytest.mark.parametrize("variant", [0, 2, 4, 6, 8, 12])
@pytest.mark.parametrize("log_n,world,log_r", [(20, 8, 8), (16, 4, 8), (12, 2, 4), (10, 8, 3), (19, 2, 8),
                                               (13, 8, 5), (11, 1, 2), (18, 4, 10)])
def test_four_step_split(log_n, world, log_r, variant):
    """Plans with R = 2^log_r != 2^floor(L/2) (tachyon_mi355x_bn254_ntt4_create_split;
    2^8 x 2^16 is split_log_r's choice for 2^24): the one-pass column NTTs
    pack 2^p columns per workgroup (variant bit 2 turns that off, same bytes;
    bit 3: the exchange twiddles computed in the pass instead of the plan's
    precomputed 29-bit table), every variant equal to the oracle's FFT slab
    and its own inverse."""
    from tachyon_amd.ntt import FourStepNtt
    if log_r == 8 and log_n >= 16:
        assert FourStepNtt.split_log_r(log_n, world) in (8, log_n // 2)
    _four_step_round_trip(log_n, world, variant, log_r)


def test_four_step_split_choice():
    """split_log_r: the fewest pass launches (passes of <= 8 stages), ties to the larger R up to C."""
    from tachyon_amd.ntt import FourStepNtt
    assert FourStepNtt.split_log_r(24, 8) == 8 and FourStepNtt.split_log_r(22, 4) == 8
    assert FourStepNtt.split_log_r(20, 2) == 8 and FourStepNtt.split_log_r(16, 1) == 8
    assert FourStepNtt.split_log_r(12, 8) == 6 and FourStepNtt.split_log_r(26, 8) == 13


def _four_step_round_trip(log_n, world, variant, log_r=None):
    import torch
    from tachyon_amd.ntt import FourStepNtt
    n = 1 << log_n
    x = O.gen_scalars("bn254_fr", 3131 + log_n, n).reshape(n, 4)
    X = x.copy().reshape(-1)
    O.fft_np(X)
    X = X.reshape(n, 4)
    stream = torch.cuda.Stream()  # the plans and every tensor op below share it
    torch.cuda.set_stream(stream)
    plans = [FourStepNtt(log_n, world, r, stream, log_r=log_r) for r in range(world)]
    for p in plans:
        p.set_variant(variant)
    m = n // world
    chunk = (m // world) * 32

    def exchange(sends):
        return [torch.cat([sends[h][r * chunk:(r + 1) * chunk] for h in range(world)]) for r in range(world)]

    def run(inputs, inverse):
        sends = [torch.empty_like(t) for t in inputs]
        for r in range(world):
            plans[r].run_stage(1, inverse, inputs[r], sends[r])
        recvs = exchange(sends)
        outs = [torch.empty_like(t) for t in inputs]
        for r in range(world):
            plans[r].run_stage(2, inverse, recvs[r], outs[r])
        torch.cuda.synchronize()
        return outs

    ins = [torch.from_numpy(np.ascontiguousarray(x[FourStepNtt.input_indices(log_n, world, r, log_r)])
                            .view(np.uint8).reshape(-1)).cuda() for r in range(world)]
    outs = run(ins, False)
    for r in range(world):
        assert outs[r].cpu().numpy().tobytes() == X[FourStepNtt.output_indices(log_n, world, r, log_r)].tobytes(), r
    back = run(outs, True)
    for r in range(world):
        assert torch.equal(back[r], ins[r]), r
    torch.cuda.set_stream(torch.cuda.default_stream())


@pytest.mark.parametrize("logn,batch,variant", [(10, 7, 1), (6, 12, 1), (6, 12, 0), (8, 64, 1), (8, 64, 5),
                                               (3, 40, 1), (5, 7, 0), (1, 6, 1)])
def test_batched_transform_device(logn, batch, variant):
    """transform_batch_device == per-array transforms (the four-step's building
    block), including one-pass sizes with several arrays per workgroup (batch
    divisible by 2^p; odd batches unpacked; variant bit 2: packing off)."""
    import torch
    n = 1 << logn
    v = O.gen_scalars("bn254_fr", 555, n * batch).reshape(batch, n * 4)
    d = domain(n)
    d.set_variant(variant)
    t = torch.from_numpy(v.view(np.uint8).reshape(-1).copy()).cuda()
    d.transform_batch_device(t.data_ptr(), batch)
    torch.cuda.synchronize()  # device-wide: covers the domain's own stream
    got = t.cpu().numpy().view(np.uint64).reshape(batch, n * 4)
    for b in range(batch):
        e = v[b].copy()
        O.fft_np(e)
        assert got[b].tobytes() == e.tobytes(), b


def test_transform_host_in_place():
    """tachyon_mi355x_..._transform_host: IcicleNTT::Run semantics (in place on
    a host vector of size() elements, natural order, the domain's coset)."""
    import ctypes
    n = 1 << 11
    coeffs = O.gen_scalars("bn254_fr", 77, n).tobytes()
    d = domain(n)
    buf = ctypes.create_string_buffer(coeffs, n * 32)
    d.transform_host(buf)
    assert buf.raw == O.fft(coeffs, n)
    d.transform_host(buf, inverse=True)
    assert buf.raw == coeffs
    five = O.field_op("bn254_fr", "to_mont", (5).to_bytes(32, "little"))
    d.set_offset(five)
    arr = np.frombuffer(coeffs, dtype=np.uint64).copy()
    d.transform_host(arr)
    assert arr.tobytes() == O.fft(coeffs, n, five)
    d.close()


@pytest.mark.parametrize("logn", [1, 2, 3, 7, 9, 11, 15, 17, 19, 21])
def test_field29_and_field32_passes_vs_oracle(logn):
    """The default 8 x 32-bit-limb passes and the 9 x 29-bit ones
    (dif29_pass_kernel, set_variant(1), and with swizzled LDS positions, 3) on
    plain and coset domains, FFT and IFFT, at
    sizes whose pass plans have odd stage counts (single radix-2 steps inside a
    pass and as the transform's last step): both bytewise equal to the oracle."""
    n = 1 << logn
    five = O.field_op("bn254_fr", "to_mont", (5).to_bytes(32, "little"))
    coeffs = O.gen_scalars("bn254_fr", 3000 + logn, n).tobytes()
    want = O.fft(coeffs, n)
    want_c = O.fft(coeffs, n, five)
    for variant in (0, 1, 3):
        d = domain(n)
        d.set_variant(variant)
        ev = d.fft(coeffs)
        assert ev == want, variant
        assert d.ifft(ev) == O.ifft(ev, n), variant
        d.set_offset(five)
        evc = d.fft(coeffs)
        assert evc == want_c, variant
        assert d.ifft(evc) == O.ifft(evc, n, five), variant
        d.close()
    with pytest.raises(ValueError):
        domain(n).set_variant(2)


def test_field29_extreme_inputs():
    """Inputs at the top of the field (every element p - 1, and p - 1 - i)
    through both pass kernels."""
    n = 1 << 12
    p = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    patterns = [(p - 1).to_bytes(32, "little") * n, b"".join(((p - 1 - i) % p).to_bytes(32, "little") for i in range(n))]
    for v in patterns:
        want = O.fft(v, n)
        for variant in (0, 1, 3):
            d = domain(n)
            d.set_variant(variant)
            assert d.fft(v) == want, variant
            assert d.ifft(want) == O.ifft(want, n), variant
            d.close()


def test_profile_pass_timings():
    """set_profile / last_timings (tools/ntt_probe.py, tools/tune_ntt.py): with
    the per-pass events on, transforms of 2^7 (one pass), 2^12 (two) and 2^17
    (three) elements on the 32-bit (variant 0) and 29-bit (1) passes still equal
    the oracle bytewise and report ceil(log_n / 8) positive pass times, none
    above the total (the events are nested, so only the rounding of the
    millisecond floats is allowed for: one microsecond); a transform after
    profiling is turned off again is unchanged."""
    for logn in (7, 12, 17):
        n = 1 << logn
        coeffs = O.gen_scalars("bn254_fr", 4000 + logn, n).tobytes()
        evals = O.fft(coeffs, n)
        back = O.ifft(evals, n)
        for variant in (0, 1):
            d = domain(n)
            d.set_variant(variant)
            d.set_profile(True)
            for run, data, want in ((d.fft, coeffs, evals), (d.ifft, evals, back)):
                assert run(data) == want, (logn, variant)
                total, passes = d.last_timings()
                assert len(passes) == (logn + 7) // 8, (logn, variant, passes)
                assert all(p > 0 for p in passes), (logn, variant, passes)
                assert total >= max(passes) - 1e-3, (logn, variant, total, passes)
            d.set_profile(False)
            assert d.fft(coeffs) == evals, (logn, variant)
            d.close()


@pytest.mark.parametrize("log_n,devices", [(4, [0, 0]), (10, [0, 0]), (13, [0, 0, 0, 0]), (16, [0] * 8),
                                           (20, [0, 0]), (11, [0, 0, 0]), (20, [0, 0, 0, 0]), (9, [0] * 5)])
def test_multi_device_domain_logical(log_n, devices):
    """One process, several devices (set_devices): the plain domain's fft / ifft,
    transform_host and transform_device run the four-step over `devices`
    (logical devices sharing the box's one GPU: the peer copies are device
    copies) -- bytewise equal to the oracle and to the single-device domain;
    a coset keeps the single device; [] restores it."""
    torch = pytest.importorskip("torch")
    n = 1 << log_n
    coeffs = O.gen_scalars("bn254_fr", 3000 + log_n, n).tobytes()
    d = domain(n)
    d.set_devices(devices)
    used = 1 << (len(devices).bit_length() - 1)  # the first 2^k ids; two parts -> the single device
    assert d.devices() == (devices[:used] if used >= 4 else [])
    ev = d.fft(coeffs)
    assert ev == O.fft(coeffs, n)
    assert d.ifft(ev) == O.ifft(ev, n)
    short = coeffs[:32 * (n // 3 + 1)]  # zero padding
    assert d.fft(short) == O.fft(short, n)
    buf = np.frombuffer(bytearray(coeffs), dtype=np.uint8).copy()
    d.transform_host(buf)
    assert buf.tobytes() == ev
    x = torch.frombuffer(bytearray(coeffs), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    d.transform_device(x.data_ptr())
    torch.cuda.synchronize()
    assert x.cpu().numpy().tobytes() == ev
    d.transform_device(x.data_ptr(), inverse=True)
    torch.cuda.synchronize()
    assert x.cpu().numpy().tobytes() == coeffs
    five = O.field_op("bn254_fr", "to_mont", (5).to_bytes(32, "little"))
    d.set_offset(five)
    assert d.fft(coeffs) == O.fft(coeffs, n, five)
    d.set_offset(O.field_op("bn254_fr", "to_mont", (1).to_bytes(32, "little")))
    d.set_devices([])
    assert d.devices() == []
    assert d.fft(coeffs) == ev
    d.close()


def test_multi_device_domain_refused():
    """Device lists the four-step cannot take leave the domain unchanged (a bad
    id, a domain too small for two parts); more devices than R = 2^floor(log n
    / 2) use the first R of them."""
    d = domain(1 << 10)
    for bad in ([0, 99], [-1, 0]):
        with pytest.raises(ValueError):
            d.set_devices(bad)
        assert d.devices() == []
    d.set_devices([0] * 64)
    assert d.devices() == [0] * 32
    d.set_devices([0, 0])  # two parts: the single device (the one-link exchange costs more)
    assert d.devices() == []
    d.set_devices([])
    tiny = domain(2)
    with pytest.raises(ValueError):
        tiny.set_devices([0, 0])
    tiny.close()
    coeffs = O.gen_scalars("bn254_fr", 77, 1 << 10).tobytes()
    assert d.fft(coeffs) == O.fft(coeffs, 1 << 10)
    d.close()
