"""The Halo2 lookup's permuted columns A' and S' on the GPU over the C-ABI: the
step between the compressed (input, table) pair and `plonk.lookup_grand_product`.

Reference: tachyon/zk/lookup/halo2/permute_expression_pair.h:29-142
(PermuteExpressionPair: the inputs sorted by canonical value, the first row of
every run of equal inputs takes that value from the table, the table's
remaining values go in ascending order to the repeated rows from the last one
down) and lookup/halo2/prover_impl.h:74-95 (both columns are then blinded
over the rows from usable_rows on, the last row included, input before table).

A pair is (A, S): one compressed input column and one compressed table column,
each n 32-byte Montgomery elements as bytes / numpy (host) or CUDA tensors.
With `out=` CUDA tensors nothing leaves the device: A' and S' go straight into
`plonk.lookup_grand_product`, `KZG.commit_lagrange` and the quotient.  Several
lookups of several circuits go into one call as one flat list.
"""
import ctypes

from ._lib import lib
from .plonk import FIELDS, _Columns, _ptr

PHASES = ("sort", "search", "ranks", "write")


class LookupPair(ctypes.Structure):
    """tachyon_mi355x_lookup_pair"""
    _fields_ = [("input", ctypes.c_void_p), ("table", ctypes.c_void_p)]


def work_bytes(n: int, count: int) -> int:
    """Device bytes one call holds with every column and output in host memory."""
    return lib().tachyon_mi355x_lookup_permute_work_bytes(n, count)


def last_timings() -> dict:
    """Milliseconds (stream events) of the last call's phases."""
    ms = (ctypes.c_float * len(PHASES))()
    lib().tachyon_mi355x_lookup_permute_last_timings(ms)
    return dict(zip(PHASES, [float(x) for x in ms]))


def _descriptors(cols, pairs):
    """The tachyon_mi355x_lookup_pair array of `pairs`; a None column is a null pointer."""
    arr = (LookupPair * max(1, len(pairs)))()
    for i, (a, s) in enumerate(pairs):
        arr[i].input = None if a is None else cols.ptr(a)
        arr[i].table = None if s is None else cols.ptr(s)
    return arr


def _outputs(cols, out, count, n):
    """(A' pointers, S' pointers, host buffers or None) of `count` pairs of outputs of n elements."""
    if out is None:
        bufs = [(ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)) for _ in range(count)]
        ptrs = [(ctypes.addressof(a), ctypes.addressof(s)) for a, s in bufs]
    else:
        if len(out) != count:
            raise ValueError("out: one (A', S') pair of tensors per lookup")
        bufs, ptrs = None, []
        for both in out:
            row = []
            for t in both:
                if t is None:
                    row.append(None)
                    continue
                p, nb, k = _ptr(t)
                if nb != 32 * n:
                    raise ValueError("out: 32 n bytes per column")
                row.append(p)
                cols.hold(k)
            ptrs.append(tuple(row))
    array = ctypes.c_void_p * max(1, count)
    return array(*[p[0] for p in ptrs]), array(*[p[1] for p in ptrs]), bufs


def permute_pairs(field, n, usable_rows, pairs, blinds, out=None):
    """tachyon_mi355x_lookup_permute_pairs.  pairs: a list of (A, S); blinds:
    per lookup the Montgomery bytes of its 2 (n - usable_rows) blinding values,
    those of A' before those of S' (a list, or all of them as one bytes
    object); out: per lookup an (A' tensor, S' tensor) pair of CUDA tensors of
    32 n bytes, to keep both on the device.  Returns (a_perm_list,
    s_perm_list, misses): per lookup A' and S' as bytes (or the `out`
    tensors) and the number of distinct values of A's usable rows found
    nowhere in S's; where that is not 0 the lookup's rows < usable_rows are
    unspecified (the reference aborts).  None on a refusal, a blinds argument
    of another length included."""
    cols = _Columns(n)
    arr = _descriptors(cols, pairs)
    out_a, out_s, bufs = _outputs(cols, out, len(pairs), n)
    bl = bytes(blinds) if isinstance(blinds, (bytes, bytearray)) else b"".join(bytes(b) for b in blinds)
    if len(bl) != 32 * 2 * max(0, n - usable_rows) * len(pairs):
        return None  # the C entry point takes a pointer alone: the length is checked here
    blbuf = ctypes.create_string_buffer(bl, max(1, len(bl)))
    misses = (ctypes.c_uint64 * max(1, len(pairs)))()
    cols.sync()
    ok = lib().tachyon_mi355x_lookup_permute_pairs(FIELDS[field], n, usable_rows, arr, len(pairs), blbuf, out_a, out_s,
                                                   misses)
    del cols
    if not ok:
        return None
    if out is not None:
        a_perm, s_perm = [o[0] for o in out], [o[1] for o in out]
    else:
        a_perm, s_perm = [a.raw[:32 * n] for a, _ in bufs], [s.raw[:32 * n] for _, s in bufs]
    return a_perm, s_perm, [int(x) for x in misses[:len(pairs)]]
