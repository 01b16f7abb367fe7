"""The drop-in IcicleNTT holder at the boundary: created without a size,
Init(group_gen) once, then FFT / IFFT of any power-of-two size the initialised
domain contains, the canonical coset given per call (icicle_ntt.h:43-87,
icicle_ntt_bn254.cc:31-101, icicle_ntt_holder.h:30-44; one holder for domain_
and extended_domain_, zk/base/entities/entity.h:83-95).

tachyon_amd.ntt.IcicleNTT (tachyon_mi355x_icicle_ntt_*) and the C++ client
bin/icicle_ntt_check (include/tachyon_mi355x_ntt_holder.h) are compared
bytewise with the oracle's CPU transforms.  Generators are computed here with
Python integers, w_N = c^((r - 1) / N) with c = 5 (BN254 Fr) / 7 (BLS12-381
Fr), never taken from the library under test; inputs are O.gen_scalars; the
cosets are 5 / 7, passed canonically."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tachyon_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = ["bn254_fr", "bls12_381_fr"]
MODULUS = {
    "bn254_fr": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "bls12_381_fr": 52435875175126190479447740508185965837690552500527637822603658699938581184513,
}
MULT_GEN = {"bn254_fr": 5, "bls12_381_fr": 7}  # the subgroup generator c, also the coset offset
CHECK_FIELD = {"bn254_fr": "bn254", "bls12_381_fr": "bls12_381"}


def to_mont(field, x: int) -> bytes:
    return O.field_op(field, "to_mont", (x % MODULUS[field]).to_bytes(32, "little"))


def from_mont(field, b: bytes) -> int:
    return int.from_bytes(O.field_op(field, "from_mont", b), "little")


def gen_int(field, log_n: int) -> int:
    r = MODULUS[field]
    assert (r - 1) % (1 << log_n) == 0
    return pow(MULT_GEN[field], (r - 1) >> log_n, r)


def gen(field, log_n: int) -> bytes:
    return to_mont(field, gen_int(field, log_n))


def coset_mont(field) -> bytes:
    return to_mont(field, MULT_GEN[field])


@functools.lru_cache(maxsize=None)
def scalars(field, seed, n) -> bytes:
    return O.gen_scalars(field, seed, n).tobytes()


@functools.lru_cache(maxsize=None)
def want_fft(field, seed, log_m, coset: bool) -> bytes:
    return O.fft(scalars(field, seed, 1 << log_m), 1 << log_m, coset_mont(field) if coset else None, field=field)


@functools.lru_cache(maxsize=None)
def want_ifft(field, seed, log_m, coset: bool) -> bytes:
    n = 1 << log_m
    out = O.ifft(scalars(field, seed, n), n, coset_mont(field) if coset else None, field=field)
    return out + bytes(32 * n - len(out))


def holder(field, log_n=None, options=None, generator=None):
    from tachyon_amd.ntt import IcicleNTT
    h = IcicleNTT(field)
    if log_n is not None or generator is not None:
        assert h.init(generator if generator is not None else gen(field, log_n), options)
        if log_n is not None:
            assert h.log_order == log_n
    return h


def run_check(tmp_path, field, log_order, steps):
    """bin/icicle_ntt_check on one holder; returns [(input, output)] per step."""
    dump = tmp_path / "icicle_ntt.bin"
    r = subprocess.run([os.path.join(BIN, "icicle_ntt_check"), "--field", CHECK_FIELD[field], "--log-order",
                        str(log_order), "--gen", gen(field, log_order).hex(), "--dump", str(dump)] + steps,
                       timeout=120, capture_output=True, text=True)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and res["field"] == field and res["calls"] and res["round_trips"], (r.stderr, res)
    raw = dump.read_bytes()
    out, pos = [], 0
    for s in steps:
        nbytes = 32 << int("".join(ch for ch in s if ch.isdigit()))
        out.append((raw[pos:pos + nbytes], raw[pos + nbytes:pos + 2 * nbytes]))
        pos += 2 * nbytes
    assert pos == len(raw)
    return out


def oracle_of(field, data, log_m, coset, inverse):
    n = 1 << log_m
    f = O.ifft if inverse else O.fft
    out = f(data, n, coset_mont(field) if coset else None, field=field)
    return out + bytes(32 * n - len(out))


def test_bls_generators_match_the_golden_roots():
    g = json.load(open(os.path.join(GOLDEN, "ntt_bls12_381_fr.json")))
    for k, v in g["roots_of_unity_mont"].items():
        assert gen("bls12_381_fr", int(k)).hex() == v, k


# ---- 1. the reference's unit-test shape (univariate_evaluation_domain_gpu_unittest.cc:51-66)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("log_n", range(5, 15))
def test_fresh_holder_fft_ifft_plain_and_coset(field, log_n):
    n, seed, c = 1 << log_n, 4100 + log_n, MULT_GEN[field]
    x = scalars(field, seed, n)
    h = holder(field, log_n)
    ev = h.fft(x, n)
    assert ev == want_fft(field, seed, log_n, False)
    assert h.ifft(ev, n) == x
    assert h.ifft(x, n) == want_ifft(field, seed, log_n, False)
    cev = h.fft(x, n, coset=c)
    assert cev == want_fft(field, seed, log_n, True) and cev != ev
    assert h.ifft(cev, n, coset=c) == x
    assert h.ifft(x, n, coset=c) == want_ifft(field, seed, log_n, True)
    # the algorithm does not change the result
    assert h.fft(x, n, algorithm=h.MIXED_RADIX) == ev and h.fft(x, n, algorithm=h.RADIX2) == ev
    h.close()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("log_n", [5, 9, 14])
def test_fresh_holder_cpp_client(tmp_path, field, log_n):
    steps = [f"f{log_n}", f"i{log_n}p", f"f{log_n}c", f"i{log_n}cp", f"i{log_n}", f"i{log_n}c"]
    for s, (inp, out) in zip(steps, run_check(tmp_path, field, log_n, steps)):
        assert out == oracle_of(field, inp, log_n, "c" in s, s[0] == "i"), s


# ---- 2. the entity pattern: ONE holder of order 4n for domain_ (n) and extended_domain_ (4n)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("log_n", [3, 7, 15])
def test_entity_pattern_one_holder_two_domains(field, log_n):
    le, n, ne, c = log_n + 2, 1 << log_n, 4 << log_n, MULT_GEN[field]
    sa, sb = 4200 + log_n, 4300 + log_n
    a, b = scalars(field, sa, n), scalars(field, sb, ne)
    h = holder(field, le)
    fa = h.fft(a, n)  # FFT n plain
    assert fa == want_fft(field, sa, log_n, False)
    fb = h.fft(b, ne, coset=c)  # FFT 4n coset
    assert fb == want_fft(field, sb, le, True)
    assert h.ifft(fb, ne, coset=c) == b  # IFFT 4n coset
    assert h.ifft(b, ne, coset=c) == want_ifft(field, sb, le, True)
    assert h.ifft(fa, n) == a  # IFFT n plain
    assert h.ifft(a, n) == want_ifft(field, sa, log_n, False)
    assert h.fft(a, n, coset=c) == want_fft(field, sa, log_n, True)  # FFT n coset
    assert h.fft(b, ne, coset=c) == fb  # FFT 4n coset again: the cached tables
    h.close()


@pytest.mark.parametrize("field", FIELDS)
def test_entity_pattern_cpp_client(tmp_path, field):
    steps = ["f7", "f9c", "i9cp", "i7", "f7c", "f9c"]
    for s, (inp, out) in zip(steps, run_check(tmp_path, field, 9, steps)):
        log_m = int("".join(ch for ch in s if ch.isdigit()))
        assert out == oracle_of(field, inp, log_m, "c" in s, s[0] == "i"), s


# ---- 3. every sub-size of one order-2^18 holder (sizes 1, 2, 4; the plan boundaries 8/9, 16/17)
@pytest.fixture(scope="module", params=FIELDS)
def holder18(request):
    h = holder(request.param, 18)
    yield request.param, h
    h.close()


@pytest.mark.parametrize("log_m", range(0, 19))
def test_every_sub_size(holder18, log_m):
    field, h = holder18
    m, seed, c = 1 << log_m, 4400 + log_m, MULT_GEN[field]
    x = scalars(field, seed, m)
    assert h.fft(x, m) == want_fft(field, seed, log_m, False)
    assert h.ifft(x, m, coset=c) == want_ifft(field, seed, log_m, True)


# ---- 4. BN254 Fr: the variant boundary (29-bit passes up to 2^20, 32-bit above)
@pytest.fixture(scope="module")
def holder21():
    h = holder("bn254_fr", 21)
    yield h
    h.close()


@pytest.mark.parametrize("log_m", [20, 21])
def test_bn254_variant_boundary(holder21, log_m):
    field, m, seed = "bn254_fr", 1 << log_m, 4500 + log_m
    x = scalars(field, seed, m)
    ev = holder21.fft(x, m)
    assert ev == want_fft(field, seed, log_m, False)
    assert holder21.ifft(ev, m) == x


# ---- 5. a generator that is not the field's default root
@pytest.mark.parametrize("field", FIELDS)
def test_non_default_generator(field):
    r, log_n, c = MODULUS[field], 10, MULT_GEN[field]
    g3 = pow(gen_int(field, log_n), 3, r)  # another primitive 2^10-th root
    h = holder(field, generator=to_mont(field, g3))
    assert h.log_order == log_n
    for log_m in (10, 6, 1):
        m = 1 << log_m
        x = scalars(field, 4600 + log_m, m)
        w = to_mont(field, pow(g3, 1 << (log_n - log_m), r))
        ev = h.fft(x, m)
        assert ev == b"".join(O.eval_at_powers(x, w, range(m), field=field)), log_m
        assert h.ifft(ev, m) == x
        # coset: coefficient j scaled by c^j first
        ints = [from_mont(field, x[32 * j:32 * j + 32]) for j in range(m)]
        scaled = b"".join(to_mont(field, v * pow(c, j, r)) for j, v in enumerate(ints))
        cev = h.fft(x, m, coset=c)
        assert cev == b"".join(O.eval_at_powers(scaled, w, range(m), field=field)), log_m
        assert h.ifft(cev, m, coset=c) == x
    h.close()


# ---- 6. options: batches on host buffers, device-resident asynchronous runs
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("log_m,batch", [(4, 3), (4, 4), (9, 2)])
def test_batched_host_buffers(field, log_m, batch):
    from tachyon_amd.ntt import IcicleNTTOptions
    m, seed, c = 1 << log_m, 4700 + 10 * log_m + batch, MULT_GEN[field]
    h = holder(field, 10, IcicleNTTOptions(batch_size=batch))
    x = scalars(field, seed, m * batch)
    ev = h.fft(x, m)
    cinv = h.ifft(x, m, coset=c)
    for b in range(batch):
        chunk = x[b * m * 32:(b + 1) * m * 32]
        assert ev[b * m * 32:(b + 1) * m * 32] == oracle_of(field, chunk, log_m, False, False), b
        assert cinv[b * m * 32:(b + 1) * m * 32] == oracle_of(field, chunk, log_m, True, True), b
    assert h.ifft(ev, m) == x
    h.close()


@pytest.mark.parametrize("field", FIELDS)
def test_device_resident_async(field):
    import torch
    from tachyon_amd.ntt import IcicleNTTOptions
    log_m, batch, c = 9, 2, MULT_GEN[field]
    m = 1 << log_m
    h = holder(field, 10, IcicleNTTOptions(batch_size=batch, are_inputs_on_device=1, are_outputs_on_device=1,
                                           is_async=1))
    x = scalars(field, 4800, m * batch)
    t = torch.from_numpy(np.frombuffer(x, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    assert h.run_ptr(t.data_ptr(), m, coset=c)
    torch.cuda.ExternalStream(h.stream).synchronize()
    got = t.cpu().numpy().tobytes()
    for b in range(batch):
        assert got[b * m * 32:(b + 1) * m * 32] == oracle_of(field, x[b * m * 32:(b + 1) * m * 32], log_m, True, False)
    assert h.run_ptr(t.data_ptr(), m, coset=c, inverse=True)
    torch.cuda.ExternalStream(h.stream).synchronize()
    assert t.cpu().numpy().tobytes() == x
    h.close()


# ---- 7. refusals: 0 returned, the buffer untouched
def refused(h, data: bytes, size, coset=1, inverse=False):
    buf = ctypes.create_string_buffer(data, len(data))
    ok = h.run_ptr(ctypes.addressof(buf), size, coset, inverse)
    assert buf.raw == data, "a refused run changed the buffer"
    return not ok


@pytest.mark.parametrize("field", FIELDS)
def test_refusals_and_lifecycle(field):
    from tachyon_amd.ntt import IcicleNTT, IcicleNTTOptions
    log_n = 10
    n, r = 1 << log_n, MODULUS[field]
    x = scalars(field, 4900, 2 * n)
    h = IcicleNTT(field)
    assert h.log_order == -1
    assert refused(h, x[:32 * 16], 16)  # run before init
    # init: not of two-power order; unsupported options
    assert not h.init(to_mont(field, 5))
    assert not h.init(to_mont(field, 0))
    assert not h.init(gen(field, log_n), IcicleNTTOptions(columns_batch=1))
    assert not h.init(gen(field, log_n), IcicleNTTOptions(ordering=1))
    assert not h.init(gen(field, log_n), IcicleNTTOptions(are_inputs_on_device=1))
    assert not h.init(gen(field, log_n), IcicleNTTOptions(are_outputs_on_device=1))
    assert not h.init(gen(field, log_n), IcicleNTTOptions(batch_size=0))
    assert h.log_order == -1
    assert h.init(gen(field, log_n))
    assert h.log_order == log_n
    assert h.init(gen(field, log_n))  # the same generator: a no-op
    assert not h.init(gen(field, log_n - 1))  # another one
    assert not h.init(to_mont(field, pow(gen_int(field, log_n), 3, r)))
    assert h.log_order == log_n
    # sizes
    assert refused(h, x[:32], 0)
    assert refused(h, x[:32 * 3], 3)
    assert refused(h, x[:32 * 48], 48)
    assert refused(h, x, 2 * n)
    # cosets
    assert refused(h, x[:32 * n], n, coset=0)
    assert refused(h, x[:32 * n], n, coset=r)
    assert refused(h, x[:32 * n], n, coset=r + 5, inverse=True)
    assert h.fft(x[:32 * n], n) == oracle_of(field, x[:32 * n], log_n, False, False)
    # release: run refuses, init works again with another order
    assert h.release()
    assert h.log_order == -1
    assert refused(h, x[:32 * n], n)
    assert h.init(gen(field, log_n + 1))
    assert h.log_order == log_n + 1
    assert h.fft(x, 2 * n, coset=MULT_GEN[field]) == oracle_of(field, x, log_n + 1, True, False)
    assert h.ifft(x[:32 * n], n) == oracle_of(field, x[:32 * n], log_n, False, True)
    h.close()


@pytest.mark.parametrize("field", FIELDS)
def test_order_one_generator_serves_size_one(field):
    h = holder(field, 0)
    x = scalars(field, 4950, 2)
    assert h.fft(x[:32], 1) == x[:32] and h.ifft(x[:32], 1, coset=MULT_GEN[field]) == x[:32]
    assert refused(h, x, 2)
    h.close()
