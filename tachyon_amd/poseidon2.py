"""Poseidon2 over BabyBear and FieldMerkleTree<BabyBear, 8> on the MI355X
(tachyon_mi355x_poseidon2_baby_bear_* / tachyon_mi355x_baby_bear_merkle_tree_*):
the hash side of TwoAdicFRI::Commit.  Elements are 4-byte little-endian
Montgomery words, a digest is 8 of them.  Every call returns True / False (or
None in place of data) on a refusal, like the reference's bool results; only a
misuse of this wrapper raises."""
import ctypes

from ._lib import lib
from .params import POSEIDON2_BB_DIGEST, POSEIDON2_BB_WIDTH, POSEIDON2_EXTERNAL

WORD = 4
DIGEST_BYTES = WORD * POSEIDON2_BB_DIGEST
STATE_BYTES = WORD * POSEIDON2_BB_WIDTH
BIT_REVERSED = 1  # TACHYON_MI355X_MERKLE_BIT_REVERSED


def _external_id(external) -> int:
    """"horizen" / "plonky3"; any other value is handed on as an id the library refuses"""
    if isinstance(external, str):
        if external not in POSEIDON2_EXTERNAL:
            raise ValueError(f"unknown external matrix {external!r}")
        return POSEIDON2_EXTERNAL[external]
    return int(external)


class Poseidon2BabyBear:
    """Poseidon2Sponge<., Poseidon2Params<BabyBear, 15, 7>>::Permute on batches
    of 16-word states."""

    def __init__(self, external="horizen"):
        self.external = _external_id(external)

    def permute_ptr(self, ptr: int, count: int, stream: int = None) -> bool:
        """In place on `count` states at `ptr`, host or device memory."""
        return lib().tachyon_mi355x_poseidon2_baby_bear_permute(self.external, ptr, count, stream) == 1

    def permute(self, states: bytes):
        """Host data: the permuted states' bytes, or None when refused."""
        data = bytes(states)
        if len(data) % STATE_BYTES:
            raise ValueError("states are 16 words of 4 bytes each")
        buf = ctypes.create_string_buffer(data, max(1, len(data)))
        ok = self.permute_ptr(ctypes.addressof(buf), len(data) // STATE_BYTES)
        return buf.raw[:len(data)] if ok else None


class FieldMerkleTree:
    """FieldMerkleTree<BabyBear, 8>::Build and FieldMerkleTreeMMCS's openings."""

    def __init__(self, external="horizen", stream: int = None):
        self._h = lib().tachyon_mi355x_baby_bear_merkle_tree_create(_external_id(external), stream)
        if not self._h:
            raise RuntimeError("FieldMerkleTree creation failed")
        self._cols = []

    def close(self):
        if self._h:
            lib().tachyon_mi355x_baby_bear_merkle_tree_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_ptr(self, mats, bit_reversed: bool = False, flags: int = None) -> bool:
        """mats: (pointer, rows, cols) per row-major matrix, host or device
        memory each.  Device matrices are referenced, not copied: keep them
        alive for open().  flags: the raw C-ABI flags instead of bit_reversed."""
        n = len(mats)
        ptrs = (ctypes.c_void_p * max(1, n))(*[m[0] for m in mats])
        rows = (ctypes.c_size_t * max(1, n))(*[m[1] for m in mats])
        cols = (ctypes.c_size_t * max(1, n))(*[m[2] for m in mats])
        if flags is None:
            flags = BIT_REVERSED if bit_reversed else 0
        ok = lib().tachyon_mi355x_baby_bear_merkle_tree_build(self._h, ptrs, rows, cols, n, flags) == 1
        if ok:
            self._cols = [int(m[2]) for m in mats]
        return ok

    def build(self, mats, bit_reversed: bool = False) -> bool:
        """mats: (bytes, rows, cols) per row-major host matrix."""
        bufs, triples = [], []
        for data, rows, cols in mats:
            data = bytes(data)
            if len(data) != rows * cols * WORD:
                raise ValueError("a matrix is rows * cols words of 4 bytes")
            bufs.append(ctypes.create_string_buffer(data, max(1, len(data))))
            triples.append((ctypes.addressof(bufs[-1]), rows, cols))
        return self.build_ptr(triples, bit_reversed)  # (host matrices are copied by the library)

    @property
    def num_layers(self) -> int:
        return lib().tachyon_mi355x_baby_bear_merkle_tree_num_layers(self._h)

    def layer_size(self, k: int) -> int:
        return lib().tachyon_mi355x_baby_bear_merkle_tree_layer_size(self._h, k)

    def layer(self, k: int):
        """Layer k's digests as bytes (layer_size(k) * 32), or None."""
        n = self.layer_size(k)
        if n == 0:
            return None
        buf = ctypes.create_string_buffer(n * DIGEST_BYTES)
        ok = lib().tachyon_mi355x_baby_bear_merkle_tree_layer(self._h, k, buf) == 1
        return buf.raw if ok else None

    def layers(self):
        """digest_layers(): every layer's bytes, the leaf layer first."""
        return [self.layer(k) for k in range(self.num_layers)]

    @property
    def root(self):
        buf = ctypes.create_string_buffer(DIGEST_BYTES)
        ok = lib().tachyon_mi355x_baby_bear_merkle_tree_root(self._h, buf) == 1
        return buf.raw if ok else None

    @property
    def layers_device_ptr(self) -> int:
        return lib().tachyon_mi355x_baby_bear_merkle_tree_layers_device_ptr(self._h)

    def open(self, index: int):
        """DoCreateOpeningProof: (the opened row's bytes per matrix in the
        build's order, the siblings' bytes from the leaf layer up), or None."""
        n = self.num_layers
        if n == 0 or index < 0:
            return None
        rows, ptrs, sib = self._opening_buffers(1, n - 1)
        if lib().tachyon_mi355x_baby_bear_merkle_tree_open(self._h, index, ptrs, sib) != 1:
            return None
        return self._openings(rows, sib, 1, n - 1)[0]

    def open_batch(self, indices):
        """open() at every index with one gather launch: a list of open()'s
        results in the indices' order, or None."""
        n, count = self.num_layers, len(indices)
        if n == 0 or any(i < 0 for i in indices):
            return None
        rows, ptrs, sib = self._opening_buffers(count, n - 1)
        idx = (ctypes.c_size_t * max(1, count))(*indices)
        if lib().tachyon_mi355x_baby_bear_merkle_tree_open_batch(self._h, idx, count, ptrs, sib) != 1:
            return None
        return self._openings(rows, sib, count, n - 1)

    def _opening_buffers(self, count, nsib):
        """rows_out's buffers, rows_out and siblings_out for `count` indices of `nsib` siblings each"""
        rows = [ctypes.create_string_buffer(max(1, count * c * WORD)) for c in self._cols]
        ptrs = (ctypes.c_void_p * max(1, len(rows)))(*[ctypes.addressof(r) for r in rows])
        return rows, ptrs, ctypes.create_string_buffer(max(1, count * nsib * DIGEST_BYTES))

    def _openings(self, rows, sib, count, nsib):
        """open()'s result per index from the filled buffers"""
        raws, sraw, out = [r.raw for r in rows], sib.raw, []
        for q in range(count):
            base = q * nsib
            out.append(([r[q * c * WORD:(q + 1) * c * WORD] for r, c in zip(raws, self._cols)],
                        [sraw[(base + k) * DIGEST_BYTES:(base + k + 1) * DIGEST_BYTES] for k in range(nsib)]))
        return out

    @property
    def last_launches(self) -> int:
        return lib().tachyon_mi355x_baby_bear_merkle_tree_last_launches(self._h)

    @property
    def stream(self) -> int:
        return lib().tachyon_mi355x_baby_bear_merkle_tree_stream(self._h)


def mul_rate(threads: int = 1 << 22, iters: int = 4096) -> float:
    """In-register bb31::mul products per second (the probe's VALU yardstick)."""
    return lib().tachyon_mi355x_baby_bear_mul_rate(threads, iters)
