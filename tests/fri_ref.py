"""The reference the FRI GPU tests compare against: BabyBear4, the prover side
of TwoAdicFRI::CreateOpeningProof, the verifier side from its own formulas, and
a DuplexChallenger, as numpy uint64 arithmetic plus Python integers.  It imports
neither the library nor the oracle.

Everything works on canonical values.  A BabyBear4 element is the last axis of
length 4 of an array: c0 + c1 x + c2 x^2 + c3 x^3 in F[x] / (x^4 - 11).  The
library stores Montgomery words; poseidon2_ref.mont_words() / from_mont_words()
convert whole arrays at the boundary.

Conventions (the reference's): a committed extension of n rows lies on the
coset 31 <w_n> in natural row order; reduced openings, folded vectors and
inverse denominators are indexed in bit-reversed order, position i belonging to
the natural row bitrev(i, log n) at x_i = 31 w_n^bitrev(i).
"""
import numpy as np

import poseidon2_ref as P2
from babybear_ref import GENERATOR, P, _powers, root_of_unity

W = 11                       # the non-residue: x^4 = 11
_P = np.uint64(P)
ORDER4 = P**4


# ---------------------------------------------------------------- BabyBear4

def ext(*c) -> np.ndarray:
    """An element from up to four canonical coefficients."""
    out = np.zeros(4, dtype=np.uint64)
    out[:len(c)] = [int(v) % P for v in c]
    return out


def from_base(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.uint64)
    out = np.zeros(a.shape + (4,), dtype=np.uint64)
    out[..., 0] = a
    return out


ZERO, ONE = ext(0), ext(1)


def e_add(a, b):
    return (np.asarray(a, dtype=np.uint64) + np.asarray(b, dtype=np.uint64)) % _P


def e_sub(a, b):
    return (np.asarray(a, dtype=np.uint64) + _P - np.asarray(b, dtype=np.uint64)) % _P


def e_neg(a):
    return (_P - np.asarray(a, dtype=np.uint64)) % _P


def e_mul_base(a, b):
    """extension x base; b broadcasts against a's leading axes"""
    return np.asarray(a, dtype=np.uint64) * np.asarray(b, dtype=np.uint64)[..., None] % _P


def e_mul(a, b):
    """The product of the polynomials, then x^(4+k) = 11 x^k."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
    conv = np.zeros(a.shape[:-1] + (7,), dtype=np.uint64)
    for i in range(4):
        for j in range(4):
            conv[..., i + j] = (conv[..., i + j] + a[..., i] * b[..., j] % _P) % _P
    out = conv[..., :4].copy()
    out[..., :3] = (out[..., :3] + np.uint64(W) * conv[..., 4:]) % _P
    return out


def e_pow(a, e: int):
    a = np.asarray(a, dtype=np.uint64)
    r = np.broadcast_to(ONE, a.shape).copy()
    while e:
        if e & 1:
            r = e_mul(r, a)
        a = e_mul(a, a)
        e >>= 1
    return r


def _b_inv(a):
    """a^(p-2) of a base-field array (0 stays 0)"""
    a = np.asarray(a, dtype=np.uint64)
    r, e = np.ones_like(a), P - 2
    while e:
        if e & 1:
            r = r * a % _P
        a = a * a % _P
        e >>= 1
    return r


def e_inv(a):
    """Through the norm to K = F[y] / (y^2 - 11), y = x^2: with A = a0 + a2 y,
    B = a1 + a3 y, N = A^2 - y B^2, a^-1 = (A - B x) / N.  0 gives 0 (the
    library's documented convention).  test_fri_ref checks it against
    a^(p^4 - 2)."""
    a = np.asarray(a, dtype=np.uint64)
    a0, a1, a2, a3 = (a[..., k] for k in range(4))
    w = np.uint64(W)
    n0 = (a0 * a0 % _P + w * (a2 * a2 % _P) % _P + (_P - np.uint64(2) * w % _P * (a1 * a3 % _P) % _P)) % _P
    n1 = (np.uint64(2) * (a0 * a2 % _P) % _P + (_P - a1 * a1 % _P) + (_P - w * (a3 * a3 % _P) % _P)) % _P
    d = (n0 * n0 % _P + (_P - w * (n1 * n1 % _P) % _P)) % _P
    di = _b_inv(d)
    i0, i1 = n0 * di % _P, (_P - n1 * di % _P) % _P
    out = np.empty_like(a)
    out[..., 0] = (a0 * i0 % _P + w * (a2 * i1 % _P) % _P) % _P
    out[..., 2] = (a0 * i1 % _P + a2 * i0 % _P) % _P
    out[..., 1] = (_P - (a1 * i0 % _P + w * (a3 * i1 % _P) % _P) % _P) % _P
    out[..., 3] = (_P - (a1 * i1 % _P + a3 * i0 % _P) % _P) % _P
    return out


def e_powers(a, n: int) -> np.ndarray:
    """[a^0 .. a^(n-1)], shape (n, 4), by doubling"""
    out = np.zeros((max(n, 1), 4), dtype=np.uint64)
    out[0] = ONE
    k, ak = 1, np.asarray(a, dtype=np.uint64)
    while k < n:
        m = min(k, n - k)
        out[k:k + m] = e_mul(out[:m], ak)
        k, ak = 2 * k, e_mul(ak, ak)
    return out[:n]


def e_sum(a, axis=0):
    return np.asarray(a, dtype=np.uint64).sum(axis=axis) % _P      # < 2^33 terms of < 2^31 fit


def to_bytes(a) -> bytes:
    """canonical elements -> the library's Montgomery words"""
    return P2.to_bytes(P2.mont_words(np.asarray(a, dtype=np.uint64).reshape(-1)))


def from_bytes(data: bytes) -> np.ndarray:
    """the library's bytes -> canonical elements, shape (n, 4)"""
    return P2.from_mont_words(P2.from_bytes(data)).reshape(-1, 4)


# ---------------------------------------------------------------- domains

def bitrev(n: int) -> np.ndarray:
    """the bit reversal of 0 .. n-1 over log2(n) bits"""
    bits = n.bit_length() - 1
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        rev |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return rev


def coset_points(n: int) -> np.ndarray:
    """x_i = 31 w_n^bitrev(i): the committed coset in the reference's order"""
    return (_powers(root_of_unity(n), n) * np.uint64(GENERATOR) % _P)[bitrev(n)]


def inverse_denominators(z, n: int) -> np.ndarray:
    """(x_i - z)^-1, i < n; None when a difference is zero (the reference CHECKs)"""
    d = e_sub(from_base(coset_points(n)), z)
    if (d == 0).all(axis=-1).any():
        return None
    return e_inv(d)


# ---------------------------------------------------------------- prover

def interpolate_coset(block, z) -> np.ndarray:
    """InterpolateCoset: the values at z of the columns' polynomials of degree
    below m, from their evaluations block[r] at 31 w_m^r (natural order)."""
    block = np.asarray(block, dtype=np.uint64)
    m = block.shape[0]
    wpow = _powers(root_of_unity(m), m)
    x = wpow * np.uint64(GENERATOR) % _P
    coef = e_mul_base(e_inv(e_sub(z, from_base(x))), wpow)                  # (m, 4)
    sums = np.stack([e_sum(coef[:, k][:, None] * block % _P) for k in range(4)], axis=-1)      # (cols, 4)
    zeroifier = e_sub(e_pow(z, m), from_base(pow(GENERATOR, m, P)))
    scale = e_mul_base(zeroifier, pow(m * pow(GENERATOR, m - 1, P), -1, P))
    return e_mul(sums, scale)


def dot_ext_powers(mat, alpha) -> np.ndarray:
    """rr[r] = sum_c alpha^c mat[r][c], natural order, shape (rows, 4)"""
    mat = np.asarray(mat, dtype=np.uint64)
    apow = e_powers(alpha, mat.shape[1])
    return np.stack([e_sum(mat * apow[:, k][None, :] % _P, axis=1) for k in range(4)], axis=-1)


def reduce_openings(alpha, rounds, log_blowup: int):
    """The first half of CreateOpeningProof.  rounds: (mats, points) per commit
    round, mats natural-order (n, cols) canonical arrays, points[m] a list of
    elements.  Returns (opened values [round][matrix][point] -> (cols, 4),
    {log n: reduced opening (n, 4) in bit-reversed order}), or None on a zero
    denominator."""
    ro, num_reduced, opened = {}, {}, []
    for mats, points in rounds:
        opened.append([])
        for mat, zs in zip(mats, points):
            mat = np.asarray(mat, dtype=np.uint64)
            n, cols = mat.shape
            log_n = n.bit_length() - 1
            ro.setdefault(log_n, np.zeros((n, 4), dtype=np.uint64))
            num_reduced.setdefault(log_n, 0)
            rr = dot_ext_powers(mat, alpha)[bitrev(n)]
            block = mat[::1 << log_blowup]
            opened[-1].append([])
            for z in zs:
                inv = inverse_denominators(z, n)
                if inv is None:
                    return None
                ys = interpolate_coset(block, z)
                reduced_ys = e_sum(e_mul(e_powers(alpha, cols), ys))
                apo = e_pow(alpha, num_reduced[log_n])
                num_reduced[log_n] += cols
                ro[log_n] = e_add(ro[log_n], e_mul(e_mul(e_sub(rr, reduced_ys), inv), apo))
                opened[-1][-1].append(ys)
    return opened, ro


def fold_matrix(beta, v) -> np.ndarray:
    """FoldMatrix on a vector of 2 rows elements viewed as rows x 2."""
    v = np.asarray(v, dtype=np.uint64).reshape(-1, 2, 4)
    rows = v.shape[0]
    w_inv = pow(root_of_unity(2 * rows), -1, P)
    half = pow(2, -1, P)
    powers = e_mul_base(e_mul_base(beta, half)[None, :], _powers(w_inv, rows)[bitrev(rows)])
    return e_add(e_mul(e_add(from_base(half), powers), v[:, 0]), e_mul(e_sub(from_base(half), powers), v[:, 1]))


def commit_phase(inputs, log_blowup: int, on_commit, external="horizen"):
    """CommitPhase.  inputs: reduced openings, largest first; on_commit(root
    (8,)) -> beta.  Returns (roots, trees' layers, the vector each tree was
    built over, the final 2^log_blowup values)."""
    folded = np.asarray(inputs[0], dtype=np.uint64)
    roots, trees, vectors = [], [], []
    while folded.shape[0] > 1 << log_blowup:
        layers = P2.build([folded.reshape(-1, 8)], external)
        roots.append(layers[-1][0])
        trees.append(layers)
        vectors.append(folded)
        folded = fold_matrix(on_commit(layers[-1][0]), folded)
        for other in inputs[1:]:
            if other.shape[0] == folded.shape[0]:
                folded = e_add(folded, other)
    return roots, trees, vectors, folded


def answer_query(index: int, trees, vectors):
    """AnswerQuery: per tree (sibling value, siblings)."""
    out = []
    for i, (layers, v) in enumerate(zip(trees, vectors)):
        index_i = index >> i
        _, siblings = P2.open_at([v.reshape(-1, 8)], layers, index_i >> 1)
        out.append((v[index_i ^ 1], siblings))
    return out


# ---------------------------------------------------------------- verifier

def fold_row(index: int, log_rows: int, beta, e0, e1):
    """FoldRow: the line through (x0, e0), (x1 = -x0, e1) at beta, x0 =
    w_(2 rows)^bitrev(index, log_rows)."""
    rev = int(format(index, "b").zfill(log_rows)[::-1], 2) if log_rows else 0
    x0 = pow(root_of_unity(2 << log_rows), rev, P)
    x1 = (P - x0) % P
    slope = e_mul_base(e_sub(e1, e0), pow((x1 - x0) % P, -1, P))
    return e_add(e0, e_mul(e_sub(beta, from_base(x0)), slope))


def verifier_reduced_openings(index: int, log_global_max: int, alpha, rounds):
    """The open_input callback of VerifyOpeningProof.  rounds: per commit round
    a list of (log n, points, opened values per point (cols, 4), the opened row
    (cols,) of the matrix at the query).  Returns {log n: value}."""
    out, pw = {}, {}
    for mats in rounds:
        for log_n, zs, values, row in mats:
            rev = index >> (log_global_max - log_n)
            rev = int(format(rev, "b").zfill(log_n)[::-1], 2) if log_n else 0
            x = GENERATOR * pow(root_of_unity(1 << log_n), rev, P) % P
            out.setdefault(log_n, ZERO.copy())
            pw.setdefault(log_n, ONE.copy())
            for z, ps_at_z in zip(zs, values):
                denom = e_inv(e_sub(from_base(x), z))
                for j in range(len(row)):
                    quotient = e_mul(e_sub(from_base(row[j]), ps_at_z[j]), denom)
                    out[log_n] = e_add(out[log_n], e_mul(pw[log_n], quotient))
                    pw[log_n] = e_mul(pw[log_n], alpha)
    return out


def verify_query(index: int, log_max: int, betas, roots, answers, reduced, external="horizen"):
    """fri::VerifyQuery: the folded evaluation, or None when an opening does
    not verify.  answers: per step (sibling value, siblings); reduced: {log n:
    value} from verifier_reduced_openings."""
    folded = ZERO.copy()
    used = 0
    for step, (beta, root, (sibling_value, siblings)) in enumerate(zip(betas, roots, answers)):
        log_folded = log_max - step - 1
        if log_folded + 1 in reduced:
            folded = e_add(folded, reduced[log_folded + 1])
            used += 1
        evals = [folded, folded]
        evals[(index ^ 1) & 1] = np.asarray(sibling_value, dtype=np.uint64)
        pair = index >> 1
        row = np.concatenate(evals)
        if not P2.verify(root, [(1 << log_folded, 8)], pair, [row], siblings, external):
            return None
        folded = fold_row(pair, log_folded, beta, evals[0], evals[1])
        index = pair
    assert used == len(reduced)
    return folded


# ---------------------------------------------------------------- challenger

class DuplexChallenger:
    """DuplexChallenger<Poseidon2, 16, 8> on canonical values."""

    def __init__(self, external="horizen"):
        self.external = external
        self.state = np.zeros(16, dtype=np.uint64)
        self.inp, self.out = [], []

    def clone(self):
        c = DuplexChallenger(self.external)
        c.state, c.inp, c.out = self.state.copy(), list(self.inp), list(self.out)
        return c

    def _duplex(self):
        self.state[:len(self.inp)] = self.inp
        self.inp = []
        self.state = P2.permute(self.state[None, :], self.external)[0]
        self.out = [int(v) for v in self.state]

    def observe(self, values):
        for v in np.asarray(values, dtype=np.uint64).reshape(-1):
            self.out = []
            self.inp.append(int(v))
            if len(self.inp) == P2.RATE:
                self._duplex()

    def sample(self) -> int:
        if self.inp or not self.out:
            self._duplex()
        return self.out.pop()

    def sample_ext(self) -> np.ndarray:
        return ext(*[self.sample() for _ in range(4)])

    def sample_bits(self, bits: int) -> int:
        return self.sample() & ((1 << bits) - 1)

    def check_witness(self, bits: int, witness: int) -> bool:
        self.observe([witness])
        return self.sample_bits(bits) == 0

    def grind(self, bits: int, batch: int = 1024) -> int:
        """The smallest witness; candidates are tried `batch` at a time.  The
        observation and the sample after it cost one permutation whether or not
        the observation fills the rate, and the sample is the state's last lane."""
        for start in range(0, P, batch):
            cand = np.arange(start, min(P, start + batch), dtype=np.uint64)
            states = np.tile(self.state, (len(cand), 1))
            states[:, :len(self.inp)] = self.inp
            states[:, len(self.inp)] = cand
            hit = np.nonzero(P2.permute(states, self.external)[:, 15] & np.uint64((1 << bits) - 1) == 0)[0]
            if len(hit):
                witness = int(cand[hit[0]])
                assert self.check_witness(bits, witness)
                return witness
        raise AssertionError("no witness")
