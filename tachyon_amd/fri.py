"""BabyBear4 and the FRI opening on the MI355X (tachyon_mi355x_baby_bear4_ops /
tachyon_mi355x_baby_bear_fri_opening_*): TwoAdicFRI::CreateOpeningProof without
its challenger.  A BabyBear4 element is 16 bytes, 4 little-endian Montgomery
words c0..c3 of F[x] / (x^4 - 11); a digest is 8 words.  The caller's transcript
samples alpha and every beta.  Every call returns True / False (or None in place
of data) on a refusal; only a misuse of this wrapper raises."""
import ctypes

from ._lib import lib
from .poseidon2 import DIGEST_BYTES, _external_id

EXT_BYTES = 16
BB4_OPS = {"add": 0, "sub": 1, "mul": 2, "square": 3, "inverse": 4}


def baby_bear4_ops_ptr(op, a: int, b: int, out: int, count: int, stream: int = None) -> bool:
    """out[i] = a[i] op b[i] on `count` elements; all host or all device memory."""
    return lib().tachyon_mi355x_baby_bear4_ops(BB4_OPS.get(op, op), a, b, out, count, stream) == 1


def baby_bear4_ops(op, a: bytes, b: bytes = None):
    """Host data: the results' bytes, or None when refused."""
    a = bytes(a)
    if len(a) % EXT_BYTES or (b is not None and len(b) != len(a)):
        raise ValueError("operands are equally many elements of 16 bytes")
    abuf = ctypes.create_string_buffer(a, max(1, len(a)))
    bbuf = ctypes.create_string_buffer(bytes(b), max(1, len(a))) if b is not None else None
    out = ctypes.create_string_buffer(max(1, len(a)))
    ok = baby_bear4_ops_ptr(op, ctypes.addressof(abuf), ctypes.addressof(bbuf) if bbuf is not None else None,
                            ctypes.addressof(out), len(a) // EXT_BYTES)
    return out.raw[:len(a)] if ok else None


def _ext(value: bytes):
    value = bytes(value)
    if len(value) != EXT_BYTES:
        raise ValueError("a BabyBear4 element is 16 bytes")
    return ctypes.create_string_buffer(value, EXT_BYTES)


class FriOpening:
    """The prover side of TwoAdicFRI::CreateOpeningProof: reduce_openings() per
    commit round, commit_phase(on_commit), answer_query(index), final_eval."""

    def __init__(self, log_blowup: int, external="horizen", stream: int = None):
        self.log_blowup = int(log_blowup)
        self._h = lib().tachyon_mi355x_baby_bear_fri_opening_create(self.log_blowup, _external_id(external), stream)
        if not self._h:
            raise RuntimeError("FriOpening creation failed")

    def close(self):
        if self._h:
            lib().tachyon_mi355x_baby_bear_fri_opening_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def begin(self, alpha: bytes) -> bool:
        return lib().tachyon_mi355x_baby_bear_fri_opening_begin(self._h, _ext(alpha)) == 1

    def add_round_ptr(self, mats, points):
        """mats: (pointer, rows, cols) per natural-order extension of one commit
        round, host or device memory each; points: per matrix a list of 16-byte
        opening points.  Returns per matrix, per point, the opened values' bytes
        (cols elements), or None.  Device matrices are referenced: keep them
        alive until the next begin()."""
        n = len(mats)
        if len(points) != n:
            raise ValueError("one list of points per matrix")
        ptrs = (ctypes.c_void_p * max(1, n))(*[m[0] for m in mats])
        rows = (ctypes.c_size_t * max(1, n))(*[m[1] for m in mats])
        cols = (ctypes.c_size_t * max(1, n))(*[m[2] for m in mats])
        pbufs = [ctypes.create_string_buffer(b"".join(bytes(_ext(z).raw) for z in ps), max(1, len(ps) * EXT_BYTES))
                 for ps in points]
        obufs = [ctypes.create_string_buffer(max(1, len(ps) * int(m[2]) * EXT_BYTES)) for ps, m in zip(points, mats)]
        pptrs = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in pbufs])
        nps = (ctypes.c_size_t * max(1, n))(*[len(ps) for ps in points])
        optrs = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in obufs])
        ok = lib().tachyon_mi355x_baby_bear_fri_opening_add_round(self._h, ptrs, rows, cols, n, pptrs, nps, optrs) == 1
        if not ok:
            return None
        out = []
        for ps, m, b in zip(points, mats, obufs):
            w = int(m[2]) * EXT_BYTES
            out.append([b.raw[p * w:(p + 1) * w] for p in range(len(ps))])
        return out

    def add_round(self, mats, points):
        """mats: (bytes, rows, cols) per row-major host matrix."""
        bufs, triples = [], []
        for data, rows, cols in mats:
            data = bytes(data)
            if len(data) != rows * cols * 4:
                raise ValueError("a matrix is rows * cols words of 4 bytes")
            bufs.append(ctypes.create_string_buffer(data, max(1, len(data))))
            triples.append((ctypes.addressof(bufs[-1]), rows, cols))
        return self.add_round_ptr(triples, points)  # (host matrices are copied by the library)

    def reduce_openings(self, alpha: bytes, rounds, device: bool = False):
        """ReduceOpenings: begin(alpha), then every round (mats, points) in
        order; the opened values by round, or None.  device: the matrices are
        (pointer, rows, cols)."""
        if not self.begin(alpha):
            return None
        out = []
        for mats, points in rounds:
            ys = self.add_round_ptr(mats, points) if device else self.add_round(mats, points)
            if ys is None:
                return None
            out.append(ys)
        return out

    @property
    def num_inputs(self) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_opening_num_inputs(self._h)

    def input_log_size(self, k: int) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_opening_input_log_size(self._h, k)

    def input(self, k: int):
        """Reduced opening k (largest first) in the reference's bit-reversed
        order, as bytes, or None."""
        if not 0 <= k < self.num_inputs:
            return None
        buf = ctypes.create_string_buffer(EXT_BYTES << self.input_log_size(k))
        ok = lib().tachyon_mi355x_baby_bear_fri_opening_input(self._h, k, buf) == 1
        return buf.raw if ok else None

    def input_device_ptr(self, k: int) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_opening_input_device_ptr(self._h, k)

    def commit(self):
        """The next commit-phase root's bytes, or None once the phase has ended
        (or when refused)."""
        buf = ctypes.create_string_buffer(DIGEST_BYTES)
        ok = lib().tachyon_mi355x_baby_bear_fri_opening_commit(self._h, buf) == 1
        return buf.raw if ok else None

    def fold(self, beta: bytes) -> bool:
        return lib().tachyon_mi355x_baby_bear_fri_opening_fold(self._h, _ext(beta)) == 1

    def commit_phase(self, on_commit):
        """CommitPhase: on_commit(root bytes) -> beta bytes is the caller's
        observe-and-sample.  Returns the roots."""
        roots = []
        while True:
            root = self.commit()
            if root is None:
                return roots
            roots.append(root)
            if not self.fold(on_commit(root)):
                raise RuntimeError("fold refused after a commit")

    @property
    def num_commits(self) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_opening_num_commits(self._h)

    def final_poly(self):
        """The last 2^log_blowup values' bytes, or None before the phase ended."""
        buf = ctypes.create_string_buffer(EXT_BYTES << self.log_blowup)
        ok = lib().tachyon_mi355x_baby_bear_fri_opening_final_poly(self._h, buf) == 1
        return buf.raw if ok else None

    @property
    def final_eval(self):
        poly = self.final_poly()
        return poly[:EXT_BYTES] if poly is not None else None

    def answer_query(self, index: int):
        """AnswerQuery: per commit-phase tree (sibling value bytes, sibling
        digests' bytes from the leaf layer up), or None."""
        if index < 0 or self.num_inputs == 0:
            return None
        log_max, commits = self.input_log_size(0), self.num_commits
        counts = [log_max - i - 1 for i in range(commits)]
        vals = ctypes.create_string_buffer(max(1, commits * EXT_BYTES))
        sibs = ctypes.create_string_buffer(max(1, sum(counts) * DIGEST_BYTES))
        if lib().tachyon_mi355x_baby_bear_fri_opening_answer_query(self._h, index, vals, sibs) != 1:
            return None
        out, at = [], 0
        for i, c in enumerate(counts):
            out.append((vals.raw[i * EXT_BYTES:(i + 1) * EXT_BYTES],
                        [sibs.raw[(at + k) * DIGEST_BYTES:(at + k + 1) * DIGEST_BYTES] for k in range(c)]))
            at += c
        return out

    @property
    def last_launches(self) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_opening_last_launches(self._h)

    @property
    def stream(self) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_opening_stream(self._h)
