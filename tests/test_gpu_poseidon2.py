"""Poseidon2 over BabyBear and FieldMerkleTree<BabyBear, 8> on the GPU at the
boundary (tachyon_amd.poseidon2 over tachyon_mi355x_poseidon2_baby_bear_* /
tachyon_mi355x_baby_bear_merkle_tree_*), compared bytewise with
tests/poseidon2_ref.py: the permutation, every digest layer of a build, the
openings, the bit-reversed leaves behind CosetLDEBatch, the refusals and the
C++ client bin/baby_bear_merkle_check.

Inputs are default_rng(seed) words in [0, p); every case also runs with all
words p - 1 and with a single non-zero word.  Device matrices sit between
guard bands of sentinel words."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import babybear_ref as B
import poseidon2_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tachyon_amd", "bin")
P = R.P
KINDS = ["random", "pm1", "single"]
EXTERNALS = ["horizen", "plonky3"]
SENTINEL = 0x5EA7BEEF
GUARD = 1024           # sentinel words before and after a device buffer


@functools.lru_cache(maxsize=None)
def words(kind: str, seed: int, count: int) -> bytes:
    """stored (Montgomery) words"""
    if kind == "random":
        w = np.random.default_rng(seed).integers(0, P, size=count, dtype=np.uint64)
    elif kind == "pm1":
        w = np.full(count, P - 1, dtype=np.uint64)
    else:
        w = np.zeros(count, dtype=np.uint64)
        w[(seed * 7919) % count] = 1 + seed % (P - 1)
    return R.to_bytes(w)


def canonical(data: bytes, cols: int) -> np.ndarray:
    return R.from_mont_words(R.from_bytes(data, cols))


def stored(x) -> bytes:
    return R.to_bytes(R.mont_words(x))


@functools.lru_cache(maxsize=None)
def ref_layers(external: str, bit_reversed: bool, *mats):
    """mats: (bytes, rows, cols); the reference's layers as stored bytes"""
    layers = R.build([canonical(d, c) for d, _, c in mats], external, bit_reversed)
    return tuple(stored(l) for l in layers)


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


def device_tree(external, mats, bit_reversed=False, stream=None):
    """Build on device copies of mats; returns (tree, device buffers)."""
    from tachyon_amd.poseidon2 import FieldMerkleTree
    t = FieldMerkleTree(external, stream)
    devs = [DeviceWords(d) for d, _, _ in mats]
    assert t.build_ptr([(dv.ptr, r, c) for dv, (_, r, c) in zip(devs, mats)], bit_reversed)
    return t, devs


def check_layers(t, want):
    assert t.num_layers == len(want)
    for k, w in enumerate(want):
        assert t.layer_size(k) == len(w) // 32
        assert t.layer(k) == w, f"layer {k}"
    assert t.root == want[-1]
    assert t.layers() == list(want)


def check_open(t, external, mats, want, index, bit_reversed=False):
    """rows and siblings against the reference, and the reference's verify walk
    wherever every opened row exists (a matrix whose height is no power of two
    has no row for the padded leaves)."""
    can = [canonical(d, c) for d, _, c in mats]
    layers = [R.from_mont_words(R.from_bytes(w, 8)) for w in want]
    rows_want, sib_want = R.open_at(can, layers, index, bit_reversed)
    got = t.open(index)
    assert got is not None
    rows, sib = got
    assert rows == [stored(r) for r in rows_want]
    assert sib == [stored(s) for s in sib_want]
    log_max = len(want) - 1
    if all((index >> (log_max - R.ceil_log2(r))) < r for _, r, _ in mats):
        opened = [canonical(r, len(r) // 4)[0] for r in rows]
        sibs = [canonical(s, 8)[0] for s in sib]
        assert R.verify(layers[-1][0], [(r, c) for _, r, c in mats], index, opened, sibs, external)


# ---- 1. the permutation: lane and workgroup edges
@pytest.mark.parametrize("external", EXTERNALS)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 1025])
def test_permute(count, external):
    from tachyon_amd.poseidon2 import Poseidon2BabyBear
    p = Poseidon2BabyBear(external)
    for kind in KINDS:
        x = words(kind, 7100 + count, 16 * count)
        want = stored(R.permute(canonical(x, 16), external))
        assert p.permute(x) == want
        d = DeviceWords(x)
        assert p.permute_ptr(d.ptr, count)
        assert d.read() == want


def test_permute_known_answer():
    """poseidon2_unittest.cc:83-104 on the device"""
    from tachyon_amd.poseidon2 import Poseidon2BabyBear
    got = Poseidon2BabyBear("horizen").permute(stored(np.arange(16)))
    assert canonical(got, 16)[0].tolist() == [
        1699737005, 296394369, 268410240, 828329642, 1491697358, 1128780676, 287184043, 1806152977,
        1380147856, 345666717, 491196631, 1875224538, 697740550, 1854502887, 1201727753, 1802410886]


# ---- 2. one matrix: the rate boundary, stale lanes, tile edges, padded layers; every layer
@pytest.mark.parametrize("cols", [1, 7, 8, 9, 16, 17, 100])
@pytest.mark.parametrize("rows", [1, 2, 3, 5, 8, 64, 65, 1000, 4096])
def test_build_one_matrix(rows, cols):
    for i, kind in enumerate(KINDS):
        externals = EXTERNALS if kind == "random" else [EXTERNALS[(i + rows + cols) % 2]]
        x = words(kind, 7200 + 13 * rows + cols, rows * cols)
        for ext in externals:
            want = ref_layers(ext, False, (x, rows, cols))
            t, devs = device_tree(ext, [(x, rows, cols)])
            check_layers(t, want)
            assert devs[0].read() == x
            assert 1 <= t.last_launches <= len(want)
            t.close()


# ---- 3. several matrices: concatenated rows, mixed heights, both input orders
def _mats(seed, dims, kind="random"):
    return tuple((words(kind, seed + i, r * c), r, c) for i, (r, c) in enumerate(dims))


MIXED = {
    "two_tallest": [(8, 3), (8, 2)],
    "three_tallest": [(65, 5), (65, 9), (65, 4)],
    "mixed_small": [(8, 3), (3, 9), (8, 2), (2, 17)],
    "mixed_large": [(1024, 10), (500, 4), (16, 33)],
    "one_row_below": [(5, 10), (1, 3), (2, 9)],
}


@pytest.mark.parametrize("reverse_order", [False, True])
@pytest.mark.parametrize("name", sorted(MIXED))
def test_several_matrices(name, reverse_order):
    dims = MIXED[name][::-1] if reverse_order else MIXED[name]
    for kind in KINDS:
        mats = _mats(7300, dims, kind)
        for ext in EXTERNALS if kind == "random" else ["horizen"]:
            want = ref_layers(ext, False, *mats)
            t, devs = device_tree(ext, mats)
            check_layers(t, want)
            size = t.layer_size(0)
            for index in sorted({0, size - 1, 7919 % size, max(r for _, r, _ in mats) - 1}):
                check_open(t, ext, mats, want, index)
            assert t.open(size) is None and t.open(1 << 40) is None
            for dv, (x, _, _) in zip(devs, mats):
                assert dv.read() == x
            t.close()


def test_cross_check_root():
    """m[i][j] = (1000003 i + 7919 j + 5) mod p, Horizen, {8x3, 3x9, 8x2, 2x17}"""
    def m(r, c):
        i, j = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
        return (stored((1000003 * i + 7919 * j + 5) % P), r, c)
    t, _ = device_tree("horizen", [m(8, 3), m(3, 9), m(8, 2), m(2, 17)])
    assert canonical(t.root, 8)[0].tolist() == [1391036921, 905385679, 1633030651, 1860389071, 953526312, 691022790,
                                                1709494378, 192750719]
    t.close()


# ---- 4. bit-reversed leaves: equal to building the row-permuted matrix
@pytest.mark.parametrize("rows", [1, 2, 8, 1024])
def test_bit_reversed_leaves(rows):
    cols = 11
    for kind in KINDS:
        x = words(kind, 7400 + rows, rows * cols)
        permuted = R.to_bytes(R.bit_reverse_rows(R.from_bytes(x, cols)))
        want = ref_layers("horizen", False, (permuted, rows, cols))
        assert want == ref_layers("horizen", True, (x, rows, cols))
        t, devs = device_tree("horizen", [(x, rows, cols)], bit_reversed=True)
        check_layers(t, want)
        for index in sorted({0, rows - 1, 5 % rows}):
            check_open(t, "horizen", [(x, rows, cols)], want, index, bit_reversed=True)
        t2, _ = device_tree("horizen", [(permuted, rows, cols)])
        check_layers(t2, want)
        t.close()
        t2.close()


def test_bit_reversed_mixed_heights():
    mats = _mats(7450, [(64, 5), (16, 9), (64, 4), (1, 3)])
    want = ref_layers("plonky3", True, *mats)
    t, _ = device_tree("plonky3", mats, bit_reversed=True)
    check_layers(t, want)
    for index in (0, 37, 63):
        check_open(t, "plonky3", mats, want, index, bit_reversed=True)
    t.close()


# ---- 5. TwoAdicFRI::Commit: CosetLDEBatch, then the bit-reversed build on the same stream
@pytest.mark.parametrize("added", [1, 2])
@pytest.mark.parametrize("cols", [3, 33])
@pytest.mark.parametrize("log_rows", [6, 10])
def test_lde_then_commit_on_one_stream(log_rows, cols, added):
    from tachyon_amd.ntt import IcicleNTT, IcicleNTTOptions
    from tachyon_amd.poseidon2 import FieldMerkleTree
    rows, shift = 1 << log_rows, 31
    out_rows = rows << added
    x = words("random", 7500 + log_rows + cols + added, rows * cols)
    lde = B.coset_lde(B.from_bytes(x, cols), added, shift)          # stored words, natural order
    reversed_lde = R.to_bytes(R.bit_reverse_rows(lde))
    want = ref_layers("horizen", False, (reversed_lde, out_rows, cols))
    h = IcicleNTT("baby_bear")
    gen = B.mont(B.root_of_unity(out_rows)).to_bytes(4, "little")
    assert h.init(gen, IcicleNTTOptions(are_inputs_on_device=1, are_outputs_on_device=1, is_async=1))
    t = FieldMerkleTree("horizen", h.stream)
    assert t.stream == h.stream
    src, dst = DeviceWords(x), DeviceWords(b"", extra_words=out_rows * cols)
    assert h.coset_lde_batch_ptr(src.ptr, rows, cols, added, shift, dst.ptr)
    assert t.build_ptr([(dst.ptr, out_rows, cols)], bit_reversed=True)   # nothing waited for in between
    check_layers(t, want)
    assert dst.read(h.stream) == B.to_bytes(lde)
    check_open(t, "horizen", [(B.to_bytes(lde), out_rows, cols)], want, 3, bit_reversed=True)
    t.close()
    h.close()


# ---- 6. one mid-size case: many workgroups, every kernel of the build
def test_mid_size():
    rows, cols = 1 << 14, 33
    x = words("random", 7600, rows * cols)
    want = ref_layers("horizen", False, (x, rows, cols))
    t, devs = device_tree("horizen", [(x, rows, cols)])
    check_layers(t, want)
    # leaf hashes, the layers above 256 digests one launch each, one for the rest
    assert t.last_launches == 1 + (14 - 9) + 1
    check_open(t, "horizen", [(x, rows, cols)], want, rows - 1)
    assert devs[0].read() == x
    t.close()


# ---- 7. host matrices, a caller's stream
def test_host_matrices_and_mixed_residency():
    from tachyon_amd.poseidon2 import FieldMerkleTree
    mats = _mats(7700, [(300, 9), (300, 2), (100, 17)])
    want = ref_layers("plonky3", False, *mats)
    t = FieldMerkleTree("plonky3")
    assert t.build(mats)
    check_layers(t, want)
    check_open(t, "plonky3", mats, want, 299)
    # the second matrix on the device, the others on the host
    d = DeviceWords(mats[1][0])
    bufs = [ctypes.create_string_buffer(m[0], len(m[0])) for m in mats]
    triples = [(ctypes.addressof(b), r, c) for b, (_, r, c) in zip(bufs, mats)]
    triples[1] = (d.ptr, mats[1][1], mats[1][2])
    assert t.build_ptr(triples)
    check_layers(t, want)
    check_open(t, "plonky3", mats, want, 17)
    t.close()


def test_callers_stream():
    import torch
    s = torch.cuda.Stream()
    mats = _mats(7800, [(1000, 17), (250, 3)])
    want = ref_layers("horizen", False, *mats)
    t, _ = device_tree("horizen", mats, stream=s.cuda_stream)
    assert t.stream == s.cuda_stream
    check_layers(t, want)
    from tachyon_amd.poseidon2 import Poseidon2BabyBear
    x = words("random", 7801, 16 * 300)
    d = DeviceWords(x)
    assert Poseidon2BabyBear("plonky3").permute_ptr(d.ptr, 300, s.cuda_stream)
    assert d.read(s.cuda_stream) == stored(R.permute(canonical(x, 16), "plonky3"))
    t.close()


# ---- 8. refusals: 0, guard bands intact, the tree still usable
def test_refusals():
    from tachyon_amd._lib import lib
    from tachyon_amd.poseidon2 import FieldMerkleTree, Poseidon2BabyBear
    L = lib()
    with pytest.raises(RuntimeError):
        FieldMerkleTree(2)
    assert not L.tachyon_mi355x_baby_bear_merkle_tree_create(-1, None)
    x = words("random", 7900, 64 * 5)
    d = DeviceWords(x)
    assert not Poseidon2BabyBear(7).permute_ptr(d.ptr, 4)
    assert not Poseidon2BabyBear("horizen").permute_ptr(None, 4)
    assert not Poseidon2BabyBear("horizen").permute_ptr(d.ptr, 0)

    t = FieldMerkleTree("horizen")
    assert t.num_layers == 0 and t.root is None and t.layer(0) is None and t.open(0) is None
    assert not t.layers_device_ptr
    good = [(d.ptr, 64, 5)]
    want = ref_layers("horizen", False, (x, 64, 5))
    assert t.build_ptr(good)
    check_layers(t, want)

    d32, d30 = DeviceWords(words("random", 7901, 32 * 3)), DeviceWords(words("random", 7902, 30 * 7))
    refused = [
        [],                                                  # count 0
        [(None, 64, 5)],                                     # a null matrix
        [(d.ptr, 0, 5)], [(d.ptr, 64, 0)],                   # rows or cols 0
        [(d.ptr, 64, 5), (d32.ptr, 32, 3), (d30.ptr, 30, 7)],  # 32 and 30 share bit_ceil
        [(d30.ptr, 30, 7), (d.ptr, 64, 5), (d32.ptr, 32, 3)],
        [(d.ptr, (1 << 30) + 1, 5)],                         # beyond the limits
    ]
    for mats in refused:
        assert not t.build_ptr(mats), mats
    assert not t.build_ptr([(d30.ptr, 30, 7)], bit_reversed=True)      # the flag with a height that is no power of two
    assert not t.build_ptr([(d.ptr, 64, 5), (d30.ptr, 30, 7)], bit_reversed=True)
    assert not t.build_ptr(good, flags=2) and not t.build_ptr(good, flags=0x80000001)   # unknown flags
    fn = L.tachyon_mi355x_baby_bear_merkle_tree_build
    one = (ctypes.c_size_t * 1)(64)
    ptrs = (ctypes.c_void_p * 1)(d.ptr)
    assert fn(None, ptrs, one, one, 1, 0) == 0
    assert fn(t._h, None, one, one, 1, 0) == 0 and fn(t._h, ptrs, None, one, 1, 0) == 0
    assert fn(t._h, ptrs, one, None, 1, 0) == 0
    # every refusal left the tree as it was
    check_layers(t, want)
    check_open(t, "horizen", [(x, 64, 5)], want, 63)
    assert t.open(64) is None and t.open(-1) is None
    assert L.tachyon_mi355x_baby_bear_merkle_tree_open(t._h, 0, None, None) == 0
    assert L.tachyon_mi355x_baby_bear_merkle_tree_root(t._h, None) == 0
    assert L.tachyon_mi355x_baby_bear_merkle_tree_layer(t._h, len(want), ctypes.create_string_buffer(32)) == 0
    assert L.tachyon_mi355x_baby_bear_merkle_tree_num_layers(None) == 0
    for dv, data in ((d, x), (d32, words("random", 7901, 32 * 3)), (d30, words("random", 7902, 30 * 7))):
        assert dv.read() == data
    # and it builds again
    assert t.build_ptr([(d30.ptr, 30, 7)])
    check_layers(t, ref_layers("horizen", False, (words("random", 7902, 30 * 7), 30, 7)))
    t.close()


# ---- 9. the C++ client of include/tachyon_mi355x_merkle_tree.h
def _splitmix_words(seed: int, n: int) -> np.ndarray:
    mask = (1 << 64) - 1
    out, x = np.empty(n, dtype=np.uint64), seed
    for i in range(n):
        x = (x + 0x9e3779b97f4a7c15) & mask
        z = x
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & mask
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & mask
        z ^= z >> 31
        out[i] = z % P
    return out


@pytest.mark.parametrize("external", EXTERNALS)
def test_cpp_client(tmp_path, external):
    dump = tmp_path / "merkle.bin"
    steps = ["b8x3,3x9,8x2,2x17", "b16x11r", "b1x5", "c5x7+1"]
    gen_word = B.mont(B.root_of_unity(1 << 6))
    r = subprocess.run([os.path.join(BIN, "baby_bear_merkle_check"), "--external", external, "--gen", str(gen_word),
                        "--dump", str(dump)] + steps, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout)
    assert out["calls"] and out["roots"] and out["steps"] == len(steps) and out["external"] == external
    data = np.frombuffer(dump.read_bytes(), dtype="<u4").astype(np.uint64)
    at = 0

    def take(n):
        nonlocal at
        assert at + n <= len(data)
        part = data[at:at + n]
        at += n
        return part

    plans = [([(8, 3), (3, 9), (8, 2), (2, 17)], False), ([(16, 11)], True), ([(1, 5)], False)]
    for s, (dims, rev) in enumerate(plans + [([(32, 7)], True)]):
        mats = []
        for m, (rows, cols) in enumerate(dims):
            w = take(rows * cols)
            assert (w == _splitmix_words(0xB2B20000 + 16 * s + m, rows * cols)).all()
            mats.append(w.reshape(rows, cols))
        if s == len(plans):           # the Commit step: the extension follows its input
            lde = B.coset_lde(mats[0], 1, 31)
            assert (take(lde.size) == lde.reshape(-1)).all()
            mats = [lde]
        can = [R.from_mont_words(m) for m in mats]
        layers = R.build(can, external, rev)
        for layer in layers:
            assert (take(layer.size) == R.mont_words(layer).reshape(-1)).all()
        index = 1 if len(layers) > 1 else 0
        rows_want, sib_want = R.open_at(can, layers, index, rev)
        for row in rows_want:
            assert (take(row.size) == R.mont_words(row)).all()
        for sib in sib_want:
            assert (take(8) == R.mont_words(sib)).all()
    assert at == len(data)
