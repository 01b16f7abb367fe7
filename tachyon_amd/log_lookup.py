"""The log-derivative lookup's prover polynomials on the GPU over the C-ABI:
the multiplicities m(X) and the grand sum phi(X).

Reference: tachyon/zk/lookup/log_derivative_halo2/prover_impl.h:99-155
(ComputeMPoly / ComputeMPolys: StableSort of the table by canonical value,
BinarySearchByKey per input row, one count per hit) and :186-316
(ComputeLogDerivatives / CreateGrandSumPoly: L = sum_k 1 / (f_k + beta) -
m / (t + beta) with the batch inverse's zero rule, its exclusive prefix sums,
phi[usable_rows] = 0, then the blinding rows of zk/base/blinder.h:33-45).

A lookup is a pair (inputs, table): a list of K >= 1 compressed input columns
and one compressed table column, each n 32-byte Montgomery elements as bytes /
numpy (host) or CUDA tensors.  beta is drawn after the m polynomials are
committed, so `m_polys` and `grand_sums` are two calls; with `out=` CUDA
tensors nothing leaves the device, ready for `KZG.commit_lagrange` and the
domain's transforms.  Several lookups of several circuits go into one call as
one flat list.
"""
import ctypes

from ._lib import lib
from .plonk import FIELDS, _Columns, _ptr

PHASES = ("sort", "count", "sums_a", "sums_b", "sums_c")


class LogLookup(ctypes.Structure):
    """tachyon_mi355x_log_lookup"""
    _fields_ = [("inputs", ctypes.POINTER(ctypes.c_void_p)), ("num_inputs", ctypes.c_size_t),
                ("table", ctypes.c_void_p)]


def tile_rows() -> int:
    """Rows one workgroup of the grand sum owns."""
    return lib().tachyon_mi355x_log_lookup_tile_rows()


def work_bytes(n: int, max_inputs: int, count: int) -> int:
    """Device bytes the larger of the two calls holds with every column staged from the host."""
    return lib().tachyon_mi355x_log_lookup_work_bytes(n, max_inputs, count)


def last_timings() -> dict:
    """Milliseconds (stream events) of the last calls' phases: sort and count
    from `m_polys`, sums_a / sums_b / sums_c from `grand_sums`."""
    ms = (ctypes.c_float * len(PHASES))()
    lib().tachyon_mi355x_log_lookup_last_timings(ms)
    return dict(zip(PHASES, [float(x) for x in ms]))


def _descriptors(cols, lookups):
    """The tachyon_mi355x_log_lookup array of `lookups`; a None column is a null pointer."""
    arr = (LogLookup * max(1, len(lookups)))()
    for i, (inputs, table) in enumerate(lookups):
        if inputs is not None:
            ptrs = (ctypes.c_void_p * max(1, len(inputs)))(*[None if f is None else cols.ptr(f) for f in inputs])
            cols.hold(ptrs)
            arr[i].inputs = ptrs
            arr[i].num_inputs = len(inputs)
        arr[i].table = None if table is None else cols.ptr(table)
    return arr


def _outputs(cols, out, count, n):
    """(pointer array, host buffers or None) of `count` outputs of n elements."""
    if out is None:
        bufs = [ctypes.create_string_buffer(max(1, 32 * n)) for _ in range(count)]
        ptrs = [ctypes.addressof(b) for b in bufs]
    else:
        if len(out) != count:
            raise ValueError("out: one tensor per lookup")
        bufs, ptrs = None, []
        for t in out:
            if t is None:
                ptrs.append(None)
                continue
            p, nb, k = _ptr(t)
            if nb != 32 * n:
                raise ValueError("out: 32 n bytes per lookup")
            ptrs.append(p)
            cols.hold(k)
    return (ctypes.c_void_p * max(1, count))(*ptrs), bufs


def m_polys(field, n, usable_rows, lookups, out=None):
    """tachyon_mi355x_log_lookup_m_polys.  lookups: a list of (inputs, table);
    out: one CUDA tensor of 32 n bytes per lookup, to keep m on the device.
    Returns (m_list, misses): per lookup m as bytes (or the `out` tensor) and
    the number of its input values found nowhere in the table's usable rows;
    None on a refusal."""
    cols = _Columns(n)
    arr = _descriptors(cols, lookups)
    outs, bufs = _outputs(cols, out, len(lookups), n)
    misses = (ctypes.c_uint64 * max(1, len(lookups)))()
    cols.sync()
    ok = lib().tachyon_mi355x_log_lookup_m_polys(FIELDS[field], n, usable_rows, arr, len(lookups), outs, misses)
    del cols
    if not ok:
        return None
    m = list(out) if out is not None else [b.raw[:32 * n] for b in bufs]
    return m, [int(x) for x in misses[:len(lookups)]]


def grand_sums(field, n, usable_rows, beta, lookups, m, blinds, out=None):
    """tachyon_mi355x_log_lookup_grand_sums.  m: per lookup its multiplicity
    column; blinds: per lookup the Montgomery bytes of its n - usable_rows - 1
    blinding values (a list, or all of them as one bytes object); out: one
    CUDA tensor of 32 n bytes per lookup.  Returns (phi_list, totals): per
    lookup phi as bytes (or the `out` tensor) and the sum of L over all usable
    rows as bytes (zero for a lookup that balances); None on a refusal, a
    blinds argument of another length included."""
    cols = _Columns(n)
    arr = _descriptors(cols, lookups)
    if m is not None and len(m) != len(lookups):
        raise ValueError("m: one column per lookup")
    mptrs = None
    if m is not None:
        mptrs = (ctypes.c_void_p * max(1, len(m)))(*[None if x is None else cols.ptr(x) for x in m])
    outs, bufs = _outputs(cols, out, len(lookups), n)
    bl = bytes(blinds) if isinstance(blinds, (bytes, bytearray)) else b"".join(bytes(b) for b in blinds)
    if len(bl) != 32 * max(0, n - usable_rows - 1) * len(lookups):
        return None  # the C entry point takes a pointer alone: the length is checked here
    blbuf = ctypes.create_string_buffer(bl, max(1, len(bl)))
    bbuf = ctypes.create_string_buffer(bytes(beta), 32) if beta is not None else None
    totals = ctypes.create_string_buffer(max(1, 32 * len(lookups)))
    cols.sync()
    ok = lib().tachyon_mi355x_log_lookup_grand_sums(FIELDS[field], n, usable_rows, bbuf, arr, mptrs, len(lookups),
                                                    blbuf, outs, totals)
    del cols
    if not ok:
        return None
    phi = list(out) if out is not None else [b.raw[:32 * n] for b in bufs]
    return phi, [totals.raw[32 * i:32 * (i + 1)] for i in range(len(lookups))]
