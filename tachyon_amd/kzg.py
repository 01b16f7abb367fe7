"""Host mirror of tachyon::crypto::KZG<G1Point, MaxDegree, Commitment> over the C-ABI.

Reference: tachyon/crypto/commitments/kzg/kzg.h -- UnsafeSetup(size[, tau])
(:169-207), N() (:167), Downsize (:210-215), Commit / CommitLagrange
(:217-258), batch commitments ResizeBatchCommitments / GetBatchCommitments
(:116-165, here `commit_batch`), g1_powers_of_tau[_lagrange] (:70-76).  The
SRS is generated and kept on the GPU (SetupForGpu, :90-114); commitments are
MSMs over it.  Scalars: Montgomery bytes / numpy (host) or CUDA tensors.

Openings: `KZG.evaluate` (batched Poly::Evaluate) and
`KZG.create_opening_proof` (GWC / SHPlonk DoCreateOpeningProof, gwc.h:83-122,
shplonk.h:84-226, with the caller's transcript), and beside them the grouping
alone (`opening_plan`, host code) and the two polynomial kernels on their own
(`poly_linear_combination`, `poly_divide_by_roots`).
"""
import ctypes
import secrets

from ._lib import KZG_SQUEEZE_FN, KZG_WRITE_FN, KzgTranscript, lib
from .msm import _ptr

CURVES = {"bn254_g1": (0, 64, "bn254_fr"), "bls12_381_g1": (2, 96, "bls12_381_fr")}


class KZG:
    def __init__(self, curve: str = "bn254_g1"):
        self.curve = curve
        self._cid, self.point_bytes, self.scalar_field = CURVES[curve]
        self._h = lib().tachyon_mi355x_kzg_create(self._cid)

    def close(self):
        if self._h:
            lib().tachyon_mi355x_kzg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def unsafe_setup(self, size: int, tau: bytes = None) -> bool:
        """tau: Montgomery bytes of the trapdoor; random (F::Random) if None."""
        if tau is None:
            from . import params as P
            r = P.FIELDS[self.scalar_field][0]
            tau = P.mont(secrets.randbelow(r), r, 4).to_bytes(32, "little")
        buf = ctypes.create_string_buffer(tau, 32)
        lib().tachyon_mi355x_kzg_unsafe_setup(self._h, size, buf)
        return True

    def N(self) -> int:
        return lib().tachyon_mi355x_kzg_n(self._h)

    def downsize(self, n: int) -> bool:
        return bool(lib().tachyon_mi355x_kzg_downsize(self._h, n))

    def _srs(self, lagrange: bool) -> bytes:
        out = ctypes.create_string_buffer(max(1, self.N() * self.point_bytes))
        lib().tachyon_mi355x_kzg_get_srs(self._h, 1 if lagrange else 0, out)
        return out.raw[:self.N() * self.point_bytes]

    def g1_powers_of_tau(self) -> bytes:
        return self._srs(False)

    def g1_powers_of_tau_lagrange(self) -> bytes:
        return self._srs(True)

    def _commit(self, scalars, lagrange: bool):
        p, n, keep = _ptr(scalars)
        out = ctypes.create_string_buffer(self.point_bytes)
        if not lib().tachyon_mi355x_kzg_commit(self._h, 1 if lagrange else 0, p, n // 32, out):
            return None
        return out.raw

    def commit(self, coeffs):
        """Commit(poly coefficients) -> affine commitment bytes, or None where
        the reference returns false (more coefficients than N, kzg.h:217-226)."""
        return self._commit(coeffs, False)

    def commit_lagrange(self, evals):
        """CommitLagrange(evaluations over the size-N domain) -> affine bytes,
        or None when |evals| > N (kzg.h:239-248)."""
        return self._commit(evals, True)

    def commit_batch(self, polys, lagrange: bool = False):
        """Batch mode (ResizeBatchCommitments + Commit(v, state, i) +
        GetBatchCommitments, kzg.h:116-165): one MSM per polynomial, the
        commitments normalised together with one inversion
        (tachyon_mi355x_kzg_commit_batch).  A list of affine bytes, or None
        when any polynomial has more than N elements."""
        if not polys:
            return []
        ptrs = [_ptr(p) for p in polys]
        arr = (ctypes.c_void_p * len(ptrs))(*[p for p, _, _ in ptrs])
        lens = (ctypes.c_size_t * len(ptrs))(*[nb // 32 for _, nb, _ in ptrs])
        out = ctypes.create_string_buffer(len(ptrs) * self.point_bytes)
        if not lib().tachyon_mi355x_kzg_commit_batch(self._h, 1 if lagrange else 0, arr, lens, len(ptrs), out):
            return None
        pb = self.point_bytes
        return [out.raw[i * pb:(i + 1) * pb] for i in range(len(ptrs))]

    def evaluate(self, polys, pairs):
        """[polys[i](z) for (i, z) in pairs] as Montgomery bytes: one batched
        device evaluation (tachyon_mi355x_kzg_evaluate_batch).  polys: host
        bytes / numpy or CUDA tensors of any lengths; z: Montgomery bytes.
        None on an index out of range."""
        keep, arr, lens = _poly_arrays(polys)
        m = len(pairs)
        idx = (ctypes.c_size_t * max(1, m))(*[_index(i) for i, _ in pairs])
        pts = ctypes.create_string_buffer(b"".join(bytes(z) for _, z in pairs), max(1, 32 * m))
        out = ctypes.create_string_buffer(max(1, 32 * m))
        if not lib().tachyon_mi355x_kzg_evaluate_batch(self._h, arr, lens, len(polys), idx, pts, m, out):
            return None
        del keep
        return [out.raw[32 * i:32 * (i + 1)] for i in range(m)]

    def create_opening_proof(self, polys, openings, transcript, scheme: str = "shplonk"):
        """CreateOpeningProof of the KZG family (gwc.h:83-122, shplonk.h:84-226)
        in one call.  openings: (polynomial index, point, claimed value) with
        Montgomery bytes; transcript: any object with squeeze_challenge() ->
        Montgomery bytes and write_to_proof(affine bytes) -> bool, called in the
        reference's order (GWC: v, every W; SHPlonk: y, v, H, u, Q).  Returns the
        affine commitments written, or None where the reference returns false
        or CHECKs (a refused argument, a failed write, Z_{T \\ 0}(u) = 0)."""
        keep, arr, lens = _poly_arrays(polys)
        m = len(openings)
        idx = (ctypes.c_size_t * max(1, m))(*[_index(o[0]) for o in openings])
        pts = ctypes.create_string_buffer(b"".join(bytes(o[1]) for o in openings), max(1, 32 * m))
        vals = ctypes.create_string_buffer(b"".join(bytes(o[2]) for o in openings), max(1, 32 * m))
        pb = self.point_bytes
        errors = []

        def squeeze(_ctx, out_fr):
            try:
                ctypes.memmove(out_fr, bytes(transcript.squeeze_challenge()), 32)
            except BaseException as e:  # an exception cannot cross the C frames
                errors.append(e)
                ctypes.memset(out_fr, 0, 32)

        def write(_ctx, affine):
            try:
                return 1 if transcript.write_to_proof(ctypes.string_at(affine, pb)) else 0
            except BaseException as e:
                errors.append(e)
                return 0

        # the wrappers live until the call returns
        cbs = KzgTranscript(KZG_SQUEEZE_FN(squeeze), KZG_WRITE_FN(write), None)
        cap = max(2, m)
        out = ctypes.create_string_buffer(cap * pb)
        count = ctypes.c_size_t(0)
        ok = lib().tachyon_mi355x_kzg_create_opening_proof(self._h, SCHEMES[scheme], arr, lens, len(polys), idx, pts,
                                                           vals, m, ctypes.byref(cbs), out, cap, ctypes.byref(count))
        del keep
        if errors:
            raise errors[0]
        if not ok:
            return None
        return [out.raw[i * pb:(i + 1) * pb] for i in range(count.value)]

    def last_open_timings(self) -> dict:
        """Milliseconds (stream events) of the last evaluate / create_opening_proof by phase."""
        ms = (ctypes.c_float * 4)()
        lib().tachyon_mi355x_kzg_last_open_timings(self._h, ms)
        return dict(zip(("evaluate", "combine", "divide", "commit"), [float(x) for x in ms]))


SCHEMES = {"gwc": 0, "shplonk": 1}
_SIZE_MAX = ctypes.c_size_t(-1).value


def _index(i):
    """A polynomial index as size_t (a negative one becomes out of range, not an exception)."""
    i = int(i)
    return i if 0 <= i <= _SIZE_MAX else _SIZE_MAX


def _poly_arrays(polys):
    ptrs = [_ptr(p) for p in polys]
    n = max(1, len(ptrs))
    arr = (ctypes.c_void_p * n)(*[p for p, _, _ in ptrs])
    lens = (ctypes.c_size_t * n)(*[nb // 32 for _, nb, _ in ptrs])
    return ptrs, arr, lens


def opening_plan(curve, scheme, lens, n, openings):
    """The grouping / validation of create_opening_proof alone (host code, no
    GPU): a list of (points, polynomial indices) per group -- GWC: one group
    per distinct point, duplicates kept; SHPlonk: one per distinct point set --
    or None on a refusal (index out of range, a length above n, conflicting
    SHPlonk values).  lens: the polynomials' lengths."""
    cid = CURVES[curve][0]
    m = len(openings)
    larr = (ctypes.c_size_t * max(1, len(lens)))(*lens)
    idx = (ctypes.c_size_t * max(1, m))(*[_index(o[0]) for o in openings])
    pts = ctypes.create_string_buffer(b"".join(bytes(o[1]) for o in openings), max(1, 32 * m))
    vals = ctypes.create_string_buffer(b"".join(bytes(o[2]) for o in openings), max(1, 32 * m))
    cap = 7 * m + 1
    out = (ctypes.c_uint64 * cap)()
    words = ctypes.c_size_t(0)
    if not lib().tachyon_mi355x_kzg_opening_plan(cid, SCHEMES[scheme], larr, len(lens), n, idx, pts, vals, m, out, cap,
                                                 ctypes.byref(words)):
        return None
    raw = bytes(out)
    groups, w = [], 1
    for _ in range(out[0]):
        k = out[w]
        points = [raw[8 * (w + 1 + 4 * j):8 * (w + 5 + 4 * j)] for j in range(k)]
        w += 1 + 4 * k
        c = out[w]
        groups.append((points, [out[w + 1 + j] for j in range(c)]))
        w += 1 + c
    return groups


def poly_linear_combination(curve, polys, coeffs, d=None, out=None):
    """sum_i coeffs[i] polys[i] - d (d off the constant term) on the device, one
    launch; polys host or device, ragged.  Returns Montgomery bytes, or fills
    `out` (a CUDA tensor of 32 x longest bytes) and returns it."""
    keep, arr, lens = _poly_arrays(polys)
    longest = max([n for n in lens[:len(polys)]], default=0)
    cbuf = ctypes.create_string_buffer(b"".join(bytes(c) for c in coeffs), max(1, 32 * len(polys)))
    dbuf = ctypes.create_string_buffer(bytes(d), 32) if d is not None else None
    res = ctypes.create_string_buffer(max(1, 32 * longest)) if out is None else None
    dst = res if out is None else _ptr(out)[0]
    if not lib().tachyon_mi355x_kzg_poly_linear_combination(CURVES[curve][0], arr, lens, cbuf, len(polys), dbuf, dst,
                                                            longest):
        return None
    del keep
    return res.raw[:32 * longest] if out is None else out


def poly_divide_by_roots(curve, poly, roots):
    """poly / prod (X - root) with the remainders dropped, the roots applied one
    after another on the device.  Returns (quotient bytes, [remainder of each
    step])."""
    p, nb, keep = _ptr(poly)
    n, k = nb // 32, len(roots)
    rbuf = ctypes.create_string_buffer(b"".join(bytes(r) for r in roots), max(1, 32 * k))
    qlen = n - min(n, k)
    q = ctypes.create_string_buffer(max(1, 32 * qlen))
    rem = ctypes.create_string_buffer(max(1, 32 * k))
    if not lib().tachyon_mi355x_kzg_poly_divide_by_roots(CURVES[curve][0], p, n, rbuf, k, q, rem):
        return None
    del keep
    return q.raw[:32 * qlen], [rem.raw[32 * i:32 * (i + 1)] for i in range(k)]
