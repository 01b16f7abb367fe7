"""Halo2 grand-product polynomials Z on the GPU over the C-ABI.

Reference: tachyon/zk/plonk/permutation/grand_product_argument.h:17-122
(CreatePoly / CreateExcessivePoly / DoCreatePoly) and its three callers --
permutation_prover_impl.h:24-86, 216-244 (BatchCreateGrandProductPolys and the
numerator / denominator callbacks), lookup/halo2/prover_impl.h:126-138,
shuffle/prover_impl.h:77 -- with the blinding rows of zk/base/blinder.h:33-45.

One definition covers the three (tachyon_mi355x_grand_product_chains): a
factor is v[j] + m t(j) + c, a poly job a numerator and a denominator factor
list, a chain an ordered list of jobs whose z[0] is the previous job's
z[usable_rows].  Columns are Montgomery bytes / numpy (host) or CUDA tensors;
with `out=` CUDA tensors Z never leaves the device, ready for
`KZG.commit_lagrange` and the domain's transforms.
"""
import ctypes

from . import params as P
from ._lib import lib
from .msm import _ptr

FIELDS = {"bn254_fr": 0, "bls12_381_fr": 2}


class GpFactor(ctypes.Structure):
    """tachyon_mi355x_gp_factor"""
    _fields_ = [("values", ctypes.c_void_p), ("table", ctypes.c_void_p), ("kind", ctypes.c_uint32),
                ("label", ctypes.c_uint32), ("m", ctypes.c_uint8 * 32), ("c", ctypes.c_uint8 * 32)]


class GpPoly(ctypes.Structure):
    """tachyon_mi355x_gp_poly"""
    _fields_ = [("num", ctypes.POINTER(GpFactor)), ("num_count", ctypes.c_size_t),
                ("den", ctypes.POINTER(GpFactor)), ("den_count", ctypes.c_size_t)]


def tile_rows() -> int:
    """Rows one workgroup owns in the ratio and apply passes."""
    return lib().tachyon_mi355x_grand_product_tile_rows()


def walk_tiles() -> int:
    """Tile products one step of the carry walk takes."""
    return lib().tachyon_mi355x_grand_product_walk_tiles()


def last_timings() -> dict:
    """Milliseconds (stream events) of the last call's passes."""
    ms = (ctypes.c_float * 3)()
    lib().tachyon_mi355x_grand_product_last_timings(ms)
    return dict(zip(("ratios", "carries", "apply"), [float(x) for x in ms]))


def _mont(field: str, x: int) -> bytes:
    r, n64, _ = P.FIELDS[field]
    return P.mont(x, r, n64).to_bytes(32, "little")


def get_delta(field: str) -> bytes:
    """GetDelta (permutation_utils.h:17-35) as Montgomery bytes: g^(2^s) for
    the field's two-adicity s; for BN254 the reference pins halo2curves'
    constant, which is 7^(2^28)."""
    r, _, g = P.FIELDS[field]
    if field == "bn254_fr":
        return _mont(field, pow(7, 1 << 28, r))
    return _mont(field, pow(g, 1 << P.two_adicity(r), r))


def factor(values, m=None, table=None, label=None, c=None):
    """One factor values[j] + m t(j) + c: t is `table` (a column), the label
    delta^label omega^j (`label`: the permutation column index), or absent."""
    if table is not None and label is not None:
        raise ValueError("a factor has a table or a label, not both")
    return {"values": values, "m": m, "table": table, "label": label, "c": c}


def _is_cuda(x):
    return getattr(x, "is_cuda", False)


class _Columns:
    """The column arguments of one call: a pointer per object (an object passed
    twice is one buffer, one upload), what keeps the buffers alive, and
    whether anything is on the device."""

    def __init__(self, n, error="a column is n 32-byte elements"):
        self.n, self.error, self.keep, self.seen, self.cuda = n, error, [], {}, False

    def ptr(self, x):
        if id(x) not in self.seen:
            p, nb, k = _ptr(x)
            if nb != 32 * self.n:
                raise ValueError(self.error)
            self.hold(k)
            self.seen[id(x)] = p
        return self.seen[id(x)]

    def hold(self, k):
        self.keep.append(k)
        self.cuda |= _is_cuda(k)

    def sync(self):
        if self.cuda:
            # the library works on a stream of its own: what produced the tensors is done first
            import torch
            torch.cuda.current_stream().synchronize()


def _fill(dst: GpFactor, f, cols):
    zero = b"\0" * 32
    dst.values = cols.ptr(f["values"])
    dst.table = None
    dst.kind, dst.label = 0, 0
    if f.get("table") is not None:
        dst.table, dst.kind = cols.ptr(f["table"]), 1
    elif f.get("label") is not None:
        dst.kind, dst.label = 2, int(f["label"])
    m = f.get("m")
    c = f.get("c")
    for dst_bytes, src in ((dst.m, m), (dst.c, c)):
        src = bytes(src) if src is not None else zero
        if len(src) != 32:
            raise ValueError("a factor's constants are 32-byte Montgomery elements")
        ctypes.memmove(dst_bytes, src, 32)


def grand_product_chains(field, n, usable_rows, chains, omega, delta, blinds, out=None):
    """tachyon_mi355x_grand_product_chains.  chains: a list of chains, each a
    list of (numerator factors, denominator factors) jobs built with
    `factor`; blinds: per job (in order over all chains) the Montgomery bytes
    of its n - usable_rows - 1 blinding values; out: one CUDA tensor of 32 n
    bytes per job, to keep Z on the device.  Returns (z_list, last_values):
    per job Z as bytes (or the `out` tensor), per chain the final
    z[usable_rows] as bytes; None on a refusal."""
    jobs = [job for chain in chains for job in chain]
    cols, polys = _Columns(n), (GpPoly * max(1, len(jobs)))()
    for i, (num, den) in enumerate(jobs):
        for side, lst in (("num", num), ("den", den)):
            arr = (GpFactor * max(1, len(lst)))()
            for k, f in enumerate(lst):
                _fill(arr[k], f, cols)
            cols.hold(arr)
            setattr(polys[i], side, arr)
            setattr(polys[i], side + "_count", len(lst))
    lens = (ctypes.c_size_t * max(1, len(chains)))(*[len(c) for c in chains])
    nblind = max(0, n - usable_rows - 1)
    bl = bytes(blinds) if isinstance(blinds, (bytes, bytearray)) else b"".join(bytes(b) for b in blinds)
    if len(bl) != 32 * nblind * len(jobs):
        raise ValueError("blinds: n - usable_rows - 1 elements per job")
    blbuf = ctypes.create_string_buffer(bl, max(1, len(bl)))
    if out is None:
        bufs = [ctypes.create_string_buffer(max(1, 32 * n)) for _ in jobs]
        ptrs = [ctypes.addressof(b) for b in bufs]
    else:
        if len(out) != len(jobs):
            raise ValueError("out: one tensor per job")
        ptrs = []
        for t in out:
            p, nb, k = _ptr(t)
            if nb != 32 * n:
                raise ValueError("out: 32 n bytes per job")
            ptrs.append(p)
            cols.hold(k)
    outs = (ctypes.c_void_p * max(1, len(jobs)))(*ptrs)
    last = ctypes.create_string_buffer(max(1, 32 * len(chains)))
    wbuf = ctypes.create_string_buffer(bytes(omega), 32) if omega is not None else None
    dbuf = ctypes.create_string_buffer(bytes(delta), 32) if delta is not None else None
    cols.sync()
    ok = lib().tachyon_mi355x_grand_product_chains(FIELDS[field], n, usable_rows, wbuf, dbuf, polys, lens, len(chains),
                                                   blbuf, outs, last)
    del cols
    if not ok:
        return None
    z = list(out) if out is not None else [b.raw[:32 * n] for b in bufs]
    return z, [last.raw[32 * i:32 * (i + 1)] for i in range(len(chains))]


def permutation_chains(values, sigmas, beta, gamma, cs_degree):
    """The chains of BatchCreateGrandProductPolys (permutation_prover_impl.h:
    24-86): per circuit one chain, job k over the columns [k L, min(m, (k+1) L))
    with L = cs_degree - 2 (ComputePermutationChunkLength); numerator
    v_i + beta delta^i omega^j + gamma, denominator v_i + beta sigma_i + gamma
    (:216-244)."""
    if cs_degree < 3:
        raise ValueError("cs_degree - 2 columns per chunk: cs_degree >= 3")
    L = cs_degree - 2
    chains = []
    for cols in values:
        if len(cols) != len(sigmas):
            raise ValueError("one value column per permutation column")
        chain = []
        for s in range(0, len(cols), L):
            idx = range(s, min(len(cols), s + L))
            chain.append(([factor(cols[i], m=beta, label=i, c=gamma) for i in idx],
                          [factor(cols[i], m=beta, table=sigmas[i], c=gamma) for i in idx]))
        chains.append(chain)
    return chains


def permutation_grand_products(values, sigmas, beta, gamma, cs_degree, n, usable_rows, omega, delta=None, blinds=(),
                               out=None, field="bn254_fr"):
    """The permutation argument's Z polynomials for one or several circuits.
    values: per circuit the list of its permutation columns' values; sigmas:
    the permuted label columns, shared; delta=None: the field's GetDelta.
    Returns (per circuit the list of its Z, per circuit the last value), with
    `out` (a flat list of tensors, circuit after circuit) in place of bytes."""
    chains = permutation_chains(values, sigmas, beta, gamma, cs_degree)
    res = grand_product_chains(field, n, usable_rows, chains, omega, get_delta(field) if delta is None else delta,
                               blinds, out)
    if res is None:
        return None
    z, last = res
    grouped, at = [], 0
    for chain in chains:
        grouped.append(z[at:at + len(chain)])
        at += len(chain)
    return grouped, last


def lookup_grand_product(A, S, A_perm, S_perm, beta, gamma, n, usable_rows, blinds=(), out=None, field="bn254_fr"):
    """The Halo2 lookup's Z (lookup/halo2/prover_impl.h:126-138): numerator
    (A + beta)(S + gamma) over the compressed input and table, denominator
    (A' + beta)(S' + gamma) over the permuted pair.  Returns (Z, last value)."""
    job = ([factor(A, c=beta), factor(S, c=gamma)], [factor(A_perm, c=beta), factor(S_perm, c=gamma)])
    return _single(field, n, usable_rows, job, blinds, out)


def shuffle_grand_product(A, S, gamma, n, usable_rows, blinds=(), out=None, field="bn254_fr"):
    """The shuffle argument's Z (shuffle/prover_impl.h:77): (A + gamma) / (S + gamma)."""
    return _single(field, n, usable_rows, ([factor(A, c=gamma)], [factor(S, c=gamma)]), blinds, out)


def _single(field, n, usable_rows, job, blinds, out):
    res = grand_product_chains(field, n, usable_rows, [[job]], None, None, blinds,
                               None if out is None else [out])
    if res is None:
        return None
    return res[0][0], res[1][0]
