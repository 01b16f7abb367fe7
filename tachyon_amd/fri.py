"""BabyBear4 and the FRI opening on the MI355X (tachyon_mi355x_baby_bear4_ops /
tachyon_mi355x_baby_bear_fri_opening_*): TwoAdicFRI::CreateOpeningProof without
its challenger.  A BabyBear4 element is 16 bytes, 4 little-endian Montgomery
words c0..c3 of F[x] / (x^4 - 11); a digest is 8 words.  The caller's transcript
samples alpha and every beta, or DuplexChallenger (the library's, with Grind on
the GPU) does in FriOpening.prove(), which is CreateOpeningProof followed by
fri::Prove in one call.  Every call returns True / False (or None in place
of data) on a refusal; only a misuse of this wrapper raises."""
import ctypes

from ._lib import FriRound, lib
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


def _point_args(points, cols):
    """add_round's points, num_points and opened_values_out for matrices of
    `cols` columns, then the output buffers and the point buffers (which the
    pointers need alive)."""
    n = len(cols)
    pbufs = [ctypes.create_string_buffer(b"".join(bytes(_ext(z).raw) for z in ps), max(1, len(ps) * EXT_BYTES))
             for ps in points]
    obufs = [ctypes.create_string_buffer(max(1, len(ps) * c * EXT_BYTES)) for ps, c in zip(points, cols)]
    pptrs = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in pbufs])
    nps = (ctypes.c_size_t * max(1, n))(*[len(ps) for ps in points])
    optrs = (ctypes.c_void_p * max(1, n))(*[ctypes.addressof(b) for b in obufs])
    return pptrs, nps, optrs, obufs, pbufs


def _opened_values(points, cols, obufs):
    """per matrix, per point, the opened values' bytes (cols elements)"""
    return [[b.raw[p * c * EXT_BYTES:(p + 1) * c * EXT_BYTES] for p in range(len(ps))]
            for ps, c, b in zip(points, cols, obufs)]


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
        widths = [int(m[2]) for m in mats]
        pptrs, nps, optrs, obufs, _keep = _point_args(points, widths)
        ok = lib().tachyon_mi355x_baby_bear_fri_opening_add_round(self._h, ptrs, rows, cols, n, pptrs, nps, optrs) == 1
        return _opened_values(points, widths, obufs) if ok else None

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
        return _split_steps(vals.raw, sibs.raw, counts)

    def answer_queries(self, indices):
        """answer_query() at every index with one launch: a list of
        answer_query()'s results in the indices' order, or None."""
        count = len(indices)
        if self.num_inputs == 0 or any(i < 0 for i in indices):
            return None
        log_max, commits = self.input_log_size(0), self.num_commits
        counts = [log_max - i - 1 for i in range(commits)]
        total = sum(counts)
        vals = ctypes.create_string_buffer(max(1, count * commits * EXT_BYTES))
        sibs = ctypes.create_string_buffer(max(1, count * total * DIGEST_BYTES))
        idx = (ctypes.c_size_t * max(1, count))(*indices)
        if lib().tachyon_mi355x_baby_bear_fri_opening_answer_queries(self._h, idx, count, vals, sibs) != 1:
            return None
        return [_split_steps(vals.raw[q * commits * EXT_BYTES:(q + 1) * commits * EXT_BYTES],
                             sibs.raw[q * total * DIGEST_BYTES:(q + 1) * total * DIGEST_BYTES], counts)
                for q in range(count)]

    def prove(self, challenger, rounds, num_queries: int, proof_of_work_bits: int):
        """CreateOpeningProof followed by fri::Prove with the transcript in
        `challenger`.  rounds: (FieldMerkleTree, points) per commit round, the
        tree built bit-reversed over device-resident natural-order extensions,
        points per matrix of the tree a list of 16-byte opening points.  Returns
        (FriProof, the opened values per round as add_round_ptr returns them),
        or None when refused."""
        n = len(rounds)
        recs = (FriRound * max(1, n))()
        keep, outs = [], []
        for r, (tree, points) in enumerate(rounds):
            if len(points) != len(tree._cols):
                raise ValueError("one list of points per matrix of the round's tree")
            pptrs, nps, optrs, obufs, pbufs = _point_args(points, tree._cols)
            recs[r] = FriRound(tree._h, pptrs, nps, optrs)
            keep.append((pbufs, pptrs, nps, optrs))
            outs.append(obufs)
        h = lib().tachyon_mi355x_baby_bear_fri_opening_prove(self._h, challenger._h, recs if n else None, n, num_queries,
                                                             proof_of_work_bits)
        if not h:
            return None
        opened = [_opened_values(points, tree._cols, obufs) for (tree, points), obufs in zip(rounds, outs)]
        proof = FriProof(h, self.input_log_size(0), [list(tree._cols) for tree, _ in rounds],
                         [tree.num_layers - 1 for tree, _ in rounds])
        return proof, opened

    @property
    def last_launches(self) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_opening_last_launches(self._h)

    @property
    def stream(self) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_opening_stream(self._h)


def _split_steps(vals: bytes, sibs: bytes, counts):
    """answer_query's result from one query's sibling values and digests"""
    out, at = [], 0
    for i, c in enumerate(counts):
        out.append((vals[i * EXT_BYTES:(i + 1) * EXT_BYTES],
                    [sibs[(at + k) * DIGEST_BYTES:(at + k + 1) * DIGEST_BYTES] for k in range(c)]))
        at += c
    return out


class FriProof:
    """fri::FRIProof and the input openings, as FriOpening.prove() returns them:
    commit_phase_commits, final_eval, pow_witness, and per query its index, its
    commit-phase steps (answer_query's form) and its input openings per round
    (FieldMerkleTree.open's form)."""

    def __init__(self, handle, log_max, cols_by_round, siblings_by_round):
        self._h, self._log_max = handle, log_max
        self._cols, self._nsib = cols_by_round, siblings_by_round

    def close(self):
        if self._h:
            lib().tachyon_mi355x_baby_bear_fri_proof_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_commits(self) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_proof_num_commits(self._h)

    @property
    def commit_phase_commits(self):
        n = self.num_commits
        buf = ctypes.create_string_buffer(max(1, n * DIGEST_BYTES))
        if lib().tachyon_mi355x_baby_bear_fri_proof_commits(self._h, buf) != 1:
            return None
        return [buf.raw[k * DIGEST_BYTES:(k + 1) * DIGEST_BYTES] for k in range(n)]

    @property
    def final_eval(self):
        buf = ctypes.create_string_buffer(EXT_BYTES)
        return buf.raw if lib().tachyon_mi355x_baby_bear_fri_proof_final_eval(self._h, buf) == 1 else None

    @property
    def pow_witness(self):
        """the witness as a Montgomery word"""
        w = ctypes.c_uint32()
        return w.value if lib().tachyon_mi355x_baby_bear_fri_proof_pow_witness(self._h, ctypes.byref(w)) == 1 else None

    @property
    def num_queries(self) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_proof_num_queries(self._h)

    def query_index(self, q: int) -> int:
        return lib().tachyon_mi355x_baby_bear_fri_proof_query_index(self._h, q)

    def query_steps(self, q: int):
        """commit_phase_openings of query q, or None"""
        commits = self.num_commits
        counts = [self._log_max - i - 1 for i in range(commits)]
        vals = ctypes.create_string_buffer(max(1, commits * EXT_BYTES))
        sibs = ctypes.create_string_buffer(max(1, sum(counts) * DIGEST_BYTES))
        if q < 0 or lib().tachyon_mi355x_baby_bear_fri_proof_query_steps(self._h, q, vals, sibs) != 1:
            return None
        return _split_steps(vals.raw, sibs.raw, counts)

    def query_input(self, q: int, round_index: int):
        """input_proof of query q for one round: (rows per matrix, siblings), or None"""
        if q < 0 or not 0 <= round_index < len(self._cols):
            return None
        cols, n = self._cols[round_index], self._nsib[round_index]
        rows = [ctypes.create_string_buffer(max(1, c * 4)) for c in cols]
        ptrs = (ctypes.c_void_p * max(1, len(rows)))(*[ctypes.addressof(r) for r in rows])
        sib = ctypes.create_string_buffer(max(1, n * DIGEST_BYTES))
        if lib().tachyon_mi355x_baby_bear_fri_proof_query_input(self._h, q, round_index, ptrs, sib) != 1:
            return None
        return ([r.raw[:c * 4] for r, c in zip(rows, cols)],
                [sib.raw[k * DIGEST_BYTES:(k + 1) * DIGEST_BYTES] for k in range(n)])


class DuplexChallenger:
    """DuplexChallenger<Poseidon2, 16, rate> over BabyBear on the host, with
    Grind on the GPU.  Words are 4-byte little-endian Montgomery words, as
    everywhere in this package."""

    def __init__(self, external="horizen", rate: int = 8, _handle=None):
        self._h = _handle or lib().tachyon_mi355x_baby_bear_duplex_challenger_create(_external_id(external), rate)
        if not self._h:
            raise RuntimeError("DuplexChallenger creation failed")

    def clone(self):
        h = lib().tachyon_mi355x_baby_bear_duplex_challenger_clone(self._h)
        if not h:
            raise RuntimeError("DuplexChallenger clone failed")
        return DuplexChallenger(_handle=h)

    def close(self):
        if self._h:
            lib().tachyon_mi355x_baby_bear_duplex_challenger_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def observe(self, values: bytes) -> bool:
        """False, with nothing observed, when a word is not below p"""
        data = bytes(values)
        if len(data) % 4:
            raise ValueError("values are words of 4 bytes")
        buf = ctypes.create_string_buffer(data, max(1, len(data)))
        return lib().tachyon_mi355x_baby_bear_duplex_challenger_observe(self._h, buf, len(data) // 4) == 1

    def sample(self, count: int = 1) -> bytes:
        buf = ctypes.create_string_buffer(max(1, 4 * count))
        if lib().tachyon_mi355x_baby_bear_duplex_challenger_sample(self._h, buf, count) != 1:
            return None
        return buf.raw[:4 * count]

    def sample_ext(self) -> bytes:
        buf = ctypes.create_string_buffer(EXT_BYTES)
        return buf.raw if lib().tachyon_mi355x_baby_bear_duplex_challenger_sample_ext(self._h, buf) == 1 else None

    def sample_bits(self, bits: int):
        """the low bits of the next sample's canonical value, or None above 30 bits"""
        out = ctypes.c_uint32()
        if bits < 0 or lib().tachyon_mi355x_baby_bear_duplex_challenger_sample_bits(self._h, bits,
                                                                                    ctypes.byref(out)) != 1:
            return None
        return out.value

    def check_witness(self, bits: int, witness: int) -> bool:
        """witness: a Montgomery word"""
        if bits < 0 or not 0 <= witness < 1 << 32:
            return False
        return lib().tachyon_mi355x_baby_bear_duplex_challenger_check_witness(self._h, bits, witness) == 1

    def state(self):
        """(the 16 state words, the input buffer, the output buffer) as bytes"""
        buf = (ctypes.c_uint32 * 50)()
        if lib().tachyon_mi355x_baby_bear_duplex_challenger_state(self._h, buf) != 1:
            return None
        raw = bytes(buf)
        return raw[:64], raw[68:68 + 4 * buf[16]], raw[136:136 + 4 * buf[33]]

    def grind(self, bits: int, stream: int = None):
        """Grind(bits) on the GPU: the smallest witness as a Montgomery word, or None"""
        out = ctypes.c_uint32()
        if bits < 0 or lib().tachyon_mi355x_baby_bear_duplex_challenger_grind(self._h, bits, ctypes.byref(out),
                                                                              stream) != 1:
            return None
        return out.value

    def grind_range(self, bits: int, begin: int, end: int, stream: int = None):
        """Grind(bits, Range) over the canonical candidates [begin, end)"""
        out = ctypes.c_uint32()
        if bits < 0 or begin < 0 or end < 0 or lib().tachyon_mi355x_baby_bear_duplex_challenger_grind_range(
                self._h, bits, begin, end, ctypes.byref(out), stream) != 1:
            return None
        return out.value
