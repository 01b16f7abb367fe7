"""BabyBear on the GPU at the boundary: IcicleNTT("baby_bear")
(tachyon_mi355x_icicle_ntt_* with field 4; IcicleNTT<BabyBear>,
icicle_ntt_baby_bear.cc:31-115), the columns layout of
Radix2EvaluationDomain::FFTBatch / CosetLDEBatch
(radix2_evaluation_domain.h:99-197) and the C++ client
bin/baby_bear_ntt_check, compared bytewise with tests/babybear_ref.py.

Generators are w_n = 31^((p-1)/n) computed in babybear_ref, never taken from
the library.  Inputs are default_rng(seed) words in [0, p); every case also
runs with all words p - 1 and with a single non-zero word, the inputs that
expose a reduction bound."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import babybear_ref as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tachyon_amd", "bin")
P = B.P
KINDS = ["random", "pm1", "single"]
SENTINEL = 0x5EA7BEEF
GUARD = 1024           # sentinel words before and after a device matrix


@functools.lru_cache(maxsize=None)
def words(kind: str, seed: int, count: int) -> bytes:
    if kind == "random":
        w = np.random.default_rng(seed).integers(0, P, size=count, dtype=np.uint64)
    elif kind == "pm1":
        w = np.full(count, P - 1, dtype=np.uint64)
    else:
        w = np.zeros(count, dtype=np.uint64)
        w[1 + (seed * 7919) % (count - 1) if count > 1 else 0] = 1 + seed % (P - 1)  # not row 0: a coset shows
    return B.to_bytes(w)


def gen(log_n: int) -> bytes:
    return B.mont(B.root_of_unity(1 << log_n)).to_bytes(4, "little")


def holder(log_n=None, options=None, generator=None):
    from tachyon_amd.ntt import IcicleNTT
    h = IcicleNTT("baby_bear")
    if log_n is not None or generator is not None:
        assert h.init(generator if generator is not None else gen(log_n), options)
        if log_n is not None:
            assert h.log_order == log_n
    return h


def ref(data: bytes, cols: int, inverse: bool, coset: int = 1, w: int = None) -> bytes:
    f = B.ifft if inverse else B.fft
    return B.to_bytes(f(B.from_bytes(data, cols), coset, w))


class DeviceWords:
    """Words on the device between two guard bands of sentinel words."""

    def __init__(self, data: bytes, extra_words: int = 0):
        import torch
        self.torch = torch
        self.n = len(data) // 4 + extra_words
        host = np.full(self.n + 2 * GUARD, SENTINEL, dtype=np.uint32)
        host[GUARD:GUARD + len(data) // 4] = np.frombuffer(data, dtype="<u4")
        self.t = torch.from_numpy(host.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + 4 * GUARD

    def read(self, stream=None) -> bytes:
        if stream is not None:
            self.torch.cuda.ExternalStream(stream).synchronize()
        raw = self.t.cpu().numpy().view(np.uint32)
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + self.n:] == SENTINEL).all(), "guard band written"
        return raw[GUARD:GUARD + self.n].astype("<u4").tobytes()


# ---- 1. the reference's unit-test shape (univariate_evaluation_domain_gpu_unittest.cc:20-66)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_n", range(5, 15))
def test_fresh_holder_fft_ifft_plain_and_coset(log_n, kind):
    n, seed = 1 << log_n, 5100 + log_n
    x = words(kind, seed, n)
    h = holder(log_n)
    ev = h.fft(x, n)
    assert ev == ref(x, 1, False)
    assert h.ifft(ev, n) == x
    assert h.ifft(x, n) == ref(x, 1, True)
    cev = h.fft(x, n, coset=31)
    assert cev == ref(x, 1, False, 31) and cev != ev
    assert h.ifft(cev, n, coset=31) == x
    assert h.ifft(x, n, coset=31) == ref(x, 1, True, 31)
    assert h.fft(x, n, algorithm=h.MIXED_RADIX) == ev and h.fft(x, n, algorithm=h.RADIX2) == ev
    assert h.fft(x, n, algorithm=h.AUTO) == ev
    h.close()


# ---- 2. every sub-size of one holder: sizes 1, 2, 4 and the one / two / three pass plans
@pytest.fixture(scope="module")
def holder21():
    h = holder(21)
    yield h
    h.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_m", range(0, 22))
def test_every_sub_size(holder21, log_m, kind):
    m = 1 << log_m
    x = words(kind, 5200 + log_m, m)
    assert holder21.fft(x, m) == ref(x, 1, False)
    assert holder21.ifft(x, m, coset=31) == ref(x, 1, True, 31)


# ---- 3. the entity pattern: one holder of order 4n serving n and 4n (entity.h:83-95)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_n", [3, 7, 15])
def test_entity_pattern(log_n, kind):
    h = holder(log_n + 2)
    for rnd in range(2):  # the second round reuses the cached coset tables
        for lm in (log_n, log_n + 2):
            m = 1 << lm
            x = words(kind, 5300 + lm + rnd, m)
            ev = h.fft(x, m)
            assert ev == ref(x, 1, False)
            cev = h.fft(x, m, coset=31)
            assert cev == ref(x, 1, False, 31)
            assert h.ifft(ev, m) == x and h.ifft(cev, m, coset=31) == x
    h.close()


# ---- 4. a non-default generator: g^3 at order 2^10
@pytest.mark.parametrize("kind", KINDS)
def test_non_default_generator(kind):
    g3 = pow(B.root_of_unity(1 << 10), 3, P)
    h = holder(generator=B.mont(g3).to_bytes(4, "little"))
    assert h.log_order == 10
    for lm in (10, 6, 1):
        m = 1 << lm
        w = pow(g3, (1 << 10) // m, P)
        x = words(kind, 5400 + lm, m)
        assert h.fft(x, m) == ref(x, 1, False, 1, w)
        assert h.ifft(x, m, coset=31) == ref(x, 1, True, 31, w)
    h.close()


# ---- 5. consecutive batches, host and device-resident-async
BATCHES = [(4, 3), (4, 4), (9, 2), (12, 5), (3, 1000)]


def ref_batches(x: bytes, m: int, batch: int, inverse: bool, coset: int) -> bytes:
    # `batch` consecutive arrays = the columns of the transposed matrix
    mat = B.from_bytes(x).reshape(batch, m).T
    f = B.ifft if inverse else B.fft
    return B.to_bytes(np.ascontiguousarray(f(mat, coset).T))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_m,batch", BATCHES)
def test_batched_host_buffers(log_m, batch, kind):
    from tachyon_amd.ntt import IcicleNTTOptions
    m = 1 << log_m
    h = holder(12, IcicleNTTOptions(batch_size=batch))
    x = words(kind, 5500 + 10 * log_m + batch, m * batch)
    ev = h.fft(x, m)
    assert ev == ref_batches(x, m, batch, False, 1)
    assert h.ifft(x, m, coset=31) == ref_batches(x, m, batch, True, 31)
    assert h.ifft(ev, m) == x
    h.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_m,batch", BATCHES)
def test_batched_device_resident_async(log_m, batch, kind):
    from tachyon_amd.ntt import IcicleNTTOptions
    m = 1 << log_m
    h = holder(12, IcicleNTTOptions(batch_size=batch, are_inputs_on_device=1, are_outputs_on_device=1, is_async=1))
    x = words(kind, 5600 + 10 * log_m + batch, m * batch)
    d = DeviceWords(x)
    assert h.run_ptr(d.ptr, m, coset=31)
    assert d.read(h.stream) == ref_batches(x, m, batch, False, 31)
    assert h.run_ptr(d.ptr, m, coset=31, inverse=True)
    assert d.read(h.stream) == x
    h.close()


# ---- 6. columns: every column against the 1-D reference, guard bands intact
SHAPES = [(1, 3), (2, 3), (3, 3), (4, 3), (10, 100), (10, 1), (11, 17), (14, 33), (9, 257), (21, 3)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_rows,cols", SHAPES)
def test_columns(log_rows, cols, kind, inverse):
    from tachyon_amd.ntt import IcicleNTTOptions
    rows = 1 << log_rows
    x = words(kind, 5700 + 31 * log_rows + cols, rows * cols)
    dev = dict(are_inputs_on_device=1, are_outputs_on_device=1)
    h_init = holder(log_rows, IcicleNTTOptions(batch_size=cols, columns_batch=1, **dev))
    h_mat = holder(log_rows, IcicleNTTOptions(**dev))
    h_host = holder(log_rows)
    for coset in (1, 31):
        want = ref(x, cols, inverse, coset)
        d = DeviceWords(x)
        assert h_init.run_ptr(d.ptr, rows, coset=coset, inverse=inverse)
        assert d.read() == want
        d = DeviceWords(x)
        assert h_mat.run_matrix_ptr(d.ptr, rows, cols, coset=coset, inverse=inverse)
        assert d.read() == want
        assert h_host.run_matrix(x, rows, cols, coset=coset, inverse=inverse) == want
    for h in (h_init, h_mat, h_host):
        h.close()


# ---- 7. CosetLDEBatch (radix2_evaluation_domain_unittest.cc:59-73)
LDE_CASES = [(1, 3, 1, 31), (2, 3, 1, 31), (3, 3, 1, 31), (4, 3, 1, 31), (10, 100, 1, 31), (5, 7, 0, 31),
             (5, 7, 2, 31), (6, 5, 3, 31), (7, 9, 1, 1), (7, 9, 2, 1), (8, 4, 1, 7), (0, 3, 2, 31), (20, 3, 1, 31)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_rows,cols,added,shift", LDE_CASES)
def test_coset_lde_batch(log_rows, cols, added, shift, kind):
    from tachyon_amd.ntt import IcicleNTTOptions
    rows = 1 << log_rows
    x = words(kind, 5800 + 17 * log_rows + cols + added, rows * cols)
    want_mat = B.coset_lde(B.from_bytes(x, cols), added, shift)
    want = B.to_bytes(want_mat)
    if shift == 1:  # the input rows reappear at stride 2^added
        assert B.to_bytes(want_mat[::1 << added]) == x
    h = holder(log_rows + added)
    assert h.coset_lde_batch(x, rows, cols, added, shift) == want
    h.close()
    hd = holder(log_rows + added, IcicleNTTOptions(are_inputs_on_device=1, are_outputs_on_device=1))
    src, dst = DeviceWords(x), DeviceWords(b"", extra_words=(rows << added) * cols)
    assert hd.coset_lde_batch_ptr(src.ptr, rows, cols, added, shift, dst.ptr)
    assert dst.read() == want
    assert src.read() == x, "CosetLDEBatch wrote its input"
    if added == 0:  # in place
        assert hd.coset_lde_batch_ptr(src.ptr, rows, cols, 0, shift, src.ptr)
        assert src.read() == want
    hd.close()


def test_coset_lde_in_place_on_the_host():
    rows, cols = 32, 7
    x = words("random", 5899, rows * cols)
    h = holder(5)
    buf = ctypes.create_string_buffer(x, len(x))
    assert h.coset_lde_batch_ptr(ctypes.addressof(buf), rows, cols, 0, 31, ctypes.addressof(buf))
    assert buf.raw == B.to_bytes(B.coset_lde(B.from_bytes(x, cols), 0, 31))
    h.close()


# ---- 8. refusals and lifecycle: 0 returned, the buffers untouched
def refused(h, data: bytes, size, coset=1, inverse=False):
    buf = ctypes.create_string_buffer(data, len(data))
    ok = h.run_ptr(ctypes.addressof(buf), size, coset, inverse)
    assert buf.raw == data, "a refused run changed the buffer"
    return not ok


def lde_refused(h, data: bytes, rows, cols, added, shift, in_place=False):
    src = ctypes.create_string_buffer(data, len(data))
    fill = bytes([0xA5]) * max(4, (len(data) << added))
    dst = src if in_place else ctypes.create_string_buffer(fill, len(fill))
    ok = h.coset_lde_batch_ptr(ctypes.addressof(src), rows, cols, added, shift, ctypes.addressof(dst))
    assert src.raw == data and (in_place or dst.raw == fill), "a refused LDE changed a buffer"
    return not ok


def test_refusals_before_and_at_init():
    from tachyon_amd.ntt import IcicleNTTOptions
    x = words("random", 5900, 16)
    h = holder()
    assert h.log_order == -1 and h.table_bytes == 0
    assert refused(h, x, 16)                                     # run before init
    assert lde_refused(h, x, 16, 1, 0, 31)
    assert not h.init(P.to_bytes(4, "little"))                   # a generator word >= p
    assert not h.init((2**32 - 1).to_bytes(4, "little"))
    assert not h.init(B.mont(31).to_bytes(4, "little"))          # order 15 * 2^27, not a power of two
    assert not h.init((0).to_bytes(4, "little"))
    assert not h.init(gen(4), IcicleNTTOptions(batch_size=0))
    assert not h.init(gen(4), IcicleNTTOptions(ordering=1))
    assert not h.init(gen(4), IcicleNTTOptions(columns_batch=2))
    assert not h.init(gen(4), IcicleNTTOptions(are_inputs_on_device=1))   # mixed residency
    assert not h.init(gen(4), IcicleNTTOptions(are_outputs_on_device=1))
    assert h.log_order == -1
    assert h.init(gen(4)) and h.log_order == 4
    assert h.init(gen(4))                                        # the same generator again: fine
    assert not h.init(gen(5)) and h.log_order == 4               # another one: refused
    assert h.fft(x, 16) == ref(x, 1, False)
    h.close()


def test_refusals_at_run():
    x = words("random", 5901, 16)
    h = holder(4)
    for size in (0, 3, 32):
        assert refused(h, x + x, size)
    for coset in (0, P, 2**32 + 1, 2**63, (1 << 64) + 1):
        assert refused(h, x, 16, coset)
        assert lde_refused(h, x[:32], 8, 1, 1, coset)
    buf = ctypes.create_string_buffer(x, len(x))
    assert not h.run_matrix_ptr(ctypes.addressof(buf), 16, 0)    # cols 0
    assert not h.run_matrix_ptr(ctypes.addressof(buf), 3, 1)
    assert not h.run_matrix_ptr(ctypes.addressof(buf), 32, 1)
    assert buf.raw == x
    assert lde_refused(h, x, 3, 1, 0, 31)                        # rows 3
    assert lde_refused(h, x, 16, 1, 1, 31)                       # rows << added above the order
    assert lde_refused(h, x, 8, 2, 2, 31)
    assert lde_refused(h, x, 8, 0, 1, 31)                        # cols 0
    assert lde_refused(h, x[:32], 8, 1, 1, P)                    # shift p
    assert lde_refused(h, x[:32], 8, 1, 1, 31, in_place=True)    # in place with added_bits 1
    assert h.fft(x, 16) == ref(x, 1, False)                      # the holder still works
    h.close()


def test_new_entries_refuse_other_fields():
    from tachyon_amd.ntt import IcicleNTT
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    h = IcicleNTT("bn254_fr")
    g = pow(5, (r - 1) >> 4, r) * pow(2, 256, r) % r
    assert h.init(g.to_bytes(32, "little"))
    data = bytes(range(256)) * 2
    buf = ctypes.create_string_buffer(data, len(data))
    out = ctypes.create_string_buffer(data, len(data))
    assert not h.run_matrix_ptr(ctypes.addressof(buf), 4, 4)
    assert not h.coset_lde_batch_ptr(ctypes.addressof(buf), 4, 4, 0, 5, ctypes.addressof(out))
    assert buf.raw == data and out.raw == data
    h.close()


def test_release_then_init_at_another_order():
    x = words("random", 5902, 64)
    h = holder(5)
    assert h.fft(x[:128], 32) == ref(x[:128], 1, False)
    assert h.release() and h.log_order == -1 and h.table_bytes == 0
    assert refused(h, x[:128], 32)
    assert h.init(gen(6)) and h.log_order == 6
    assert h.fft(x, 64) == ref(x, 1, False)
    h.close()


def test_order_one_serves_size_one_only():
    h = holder(0)
    x = words("random", 5903, 2)
    assert h.fft(x[:4], 1) == x[:4] and h.ifft(x[:4], 1, coset=31) == x[:4]
    assert refused(h, x, 2)
    h.close()


def test_table_bytes_at_the_largest_order():
    """Init only: the two-level tables at LN = 27 stay far below one N/2-entry
    table (2^28 bytes); no transform at that size."""
    h = holder(27)
    assert 0 < h.table_bytes < 2**28
    x = words("random", 5904, 16)
    assert h.fft(x, 16) == ref(x, 1, False)
    h.close()


# ---- 9. the C++ client on include/tachyon_mi355x_ntt_holder.h alone
def test_cpp_client(tmp_path):
    steps = "f9 i9 f9c i9c m6x3 m10x100 l4x3+1 l10x100+1".split()
    dump = tmp_path / "baby_bear_ntt.bin"
    gen_word = int.from_bytes(gen(11), "little")
    r = subprocess.run([os.path.join(BIN, "baby_bear_ntt_check"), "--gen", str(gen_word), "--dump", str(dump)] + steps,
                       timeout=120, capture_output=True, text=True)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and res["log_order"] == 11 and res["calls"] and res["release"], (r.stderr, res)
    raw, pos = dump.read_bytes(), 0
    for s in steps:
        kind, rest = s[0], s[1:]
        if kind in "fi":
            coset = rest.endswith("c")
            n_in = n_out = 1 << int(rest.rstrip("c"))
            cols = 1
        else:
            lm, rest = rest.split("x")
            cols, added = (rest.split("+") + ["0"])[:2]
            cols, added = int(cols), int(added)
            n_in = (1 << int(lm)) * cols
            n_out = n_in << added
        x, y = raw[pos:pos + 4 * n_in], raw[pos + 4 * n_in:pos + 4 * (n_in + n_out)]
        pos += 4 * (n_in + n_out)
        if kind == "l":
            want = B.to_bytes(B.coset_lde(B.from_bytes(x, cols), added, 31))
        else:
            want = ref(x, cols, kind == "i", 31 if kind in "fi" and coset else 1)
        assert y == want, s
    assert pos == len(raw)
