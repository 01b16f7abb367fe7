"""The DuplexChallenger's grind on the GPU, the batched openings and the whole
opening proof in one call (tachyon_amd.fri.DuplexChallenger / FriOpening.prove /
FriOpening.answer_queries, FieldMerkleTree.open_batch), compared bytewise with
tests/fri_ref.py and tests/poseidon2_ref.py, which import neither the library
nor the oracle.  There are no tolerances: every result is a canonical field
element.

Paths covered:
  grind      the candidate's slot 0, 3 and 7 (7 fills the rate), an output buffer
             that the observation clears, bits 0 (every candidate hits), 1, 8
             and 12 (all inside the first chunk of 2^16 candidates) and a 16-bit
             case whose witness lies beyond it, so later chunks run; ranges of
             one candidate, up to p, without a witness, and the last 4096
             candidates below p
  gathers    trees with and without the bit-reversed flag, a height that is no
             power of two (rows that open as zeros), rows of 1, 5, 33 columns
             (part of a block's 256 lanes) and of 257 and 300 (a lane copies a
             second column), every index, repeats, shuffled order; each
             batched answer is compared with the single-index call, which is
             the same kernel at count 1, and with poseidon2_ref / fri_ref
  count 1    the single-index calls as batches of one: the edges of the index
             range, launch counts, refusals that leave the caller's buffers
             alone, an opening without a commit-phase tree, a one-leaf tree
  the proof  the reference unit test's shapes (duplicate query indices occur)
             and a two-round, four-matrix shape with two points, no point, 33
             queries and 12 bits
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import babybear_ref as B
import fri_ref as F
import poseidon2_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tachyon_amd", "bin")
P = R.P
EXTERNALS = ["horizen", "plonky3"]


def stored(x) -> bytes:
    return R.to_bytes(R.mont_words(np.asarray(x, dtype=np.uint64).reshape(-1)))


def canon(data: bytes) -> np.ndarray:
    return R.from_mont_words(R.from_bytes(data))


def mont(v: int) -> int:
    return int(R.mont_words([v])[0])


def rand_words(seed: int, count: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, P, size=count, dtype=np.uint64)


def same_state(ch, ref) -> bool:
    st, inp, out = ch.state()
    return (canon(st) == ref.state).all() and list(canon(inp)) == ref.inp and list(canon(out)) == ref.out


def pair(external):
    """the library's challenger and fri_ref's, rate 8"""
    from tachyon_amd.fri import DuplexChallenger
    return DuplexChallenger(external, 8), F.DuplexChallenger(external)


def observe_both(ch, ref, values):
    assert ch.observe(stored(values))
    ref.observe(values)


def ref_scan(ref, bits: int, begin: int, end: int):
    """the smallest witness in [begin, end) by fri_ref's rule (one permutation
    per candidate, the sample is lane 15), or None; ref is not advanced"""
    for start in range(begin, end, 4096):
        cand = np.arange(start, min(end, start + 4096), dtype=np.uint64)
        states = np.tile(ref.state, (len(cand), 1))
        states[:, :len(ref.inp)] = ref.inp
        states[:, len(ref.inp)] = cand
        hit = np.nonzero(R.permute(states, ref.external)[:, 15] & np.uint64((1 << bits) - 1) == 0)[0]
        if len(hit):
            return int(cand[hit[0]])
    return None


class DeviceWords:
    """Words on the device (kept alive by the caller)."""

    def __init__(self, data: bytes):
        import torch
        self.t = torch.from_numpy(np.frombuffer(data, dtype="<u4").view(np.int32).copy()).cuda()
        torch.cuda.synchronize()

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()


# ---- 1. the host permutation against the device's
@pytest.mark.parametrize("external", EXTERNALS)
def test_host_poseidon2_equals_device(external):
    from tachyon_amd.fri import DuplexChallenger
    from tachyon_amd.poseidon2 import Poseidon2BabyBear
    states = stored(rand_words(4100, 4096 * 16))
    device = Poseidon2BabyBear(external).permute(states)
    assert device is not None
    for i in range(4096):
        ch = DuplexChallenger(external, 16)          # 16 observations: one duplex of exactly these words
        assert ch.observe(states[64 * i:64 * (i + 1)])
        assert ch.state()[0] == device[64 * i:64 * (i + 1)], i
        ch.close()


# ---- 2. grind against fri_ref.grind
@pytest.mark.parametrize("fill", ["empty", "outputs", "k3", "k7"])
@pytest.mark.parametrize("external", EXTERNALS)
def test_grind_smallest_witness(external, fill):
    for bits in (0, 1, 8, 12):
        ch, ref = pair(external)
        if fill != "empty":
            observe_both(ch, ref, rand_words(4200 + bits, 8))         # a duplex: 16 outputs
            assert int(canon(ch.sample())[0]) == ref.sample()         # 15 left
            assert len(ch.state()[2]) == 60
        if fill in ("k3", "k7"):
            observe_both(ch, ref, rand_words(4300 + bits, int(fill[1])))
            assert len(ch.state()[1]) == 4 * int(fill[1]) and ch.state()[2] == b""
        want = ref.grind(bits)                                        # advances ref by its check_witness
        assert ch.grind(bits) == mont(want), (fill, bits)
        assert same_state(ch, ref)
        assert int(canon(ch.sample())[0]) == ref.sample()


def fixed_transcript():
    ch, ref = pair("horizen")
    observe_both(ch, ref, np.arange(1, 12))
    return ch, ref


def test_grind_beyond_the_first_chunk():
    """16 bits from a transcript whose witness lies beyond 2^16: the first
    launch finds nothing and the later chunks run"""
    ch, ref = fixed_transcript()
    want = ref.grind(16)
    assert want >= 1 << 16
    assert ch.grind(16) == mont(want)
    assert same_state(ch, ref)


def test_grind_range():
    ch, ref = fixed_transcript()
    start = ch.state()
    w = ref_scan(ref, 12, 0, P)
    assert w == ref.clone().grind(12) and w > 0

    one = ch.clone()
    assert one.grind_range(12, w, w + 1) == mont(w)
    after = ref.clone()
    assert after.check_witness(12, w) and same_state(one, after)

    nxt = ref_scan(ref, 12, w + 1, w + 1 + (1 << 17))
    assert nxt is not None
    two = ch.clone()
    assert two.grind_range(12, w + 1, P) == mont(nxt)
    after = ref.clone()
    assert after.check_witness(12, nxt) and same_state(two, after)

    assert ch.grind_range(12, 0, w) is None                  # no witness below the smallest
    assert ch.grind_range(12, 0, P + 1) is None and ch.grind_range(12, 5, 5) is None
    assert ch.grind_range(31, 0, P) is None
    assert ch.state() == start and same_state(ch, ref)

    top = ref_scan(ref, 4, P - 4096, P)                      # the Montgomery conversion near p
    assert top is not None
    assert ch.grind_range(4, P - 4096, P) == mont(top)
    assert ref.check_witness(4, top) and same_state(ch, ref)


# ---- 3. open_batch against open
def batch_indices(n: int, seed: int):
    idx = list(range(n)) + [0, n - 1, n // 2, n // 2, 3 % n, 3 % n]
    np.random.default_rng(seed).shuffle(idx)
    return [int(i) for i in idx]


def verify_padded(root, dims, index: int, opened, siblings, external) -> bool:
    """poseidon2_ref.verify's walk from the opened rows up to the root, with
    FieldMerkleTree::Build's rule for a height that is no power of two: the
    digest of a row past a matrix's height is the zero digest, not a hash"""
    rest = sorted(range(len(dims)), key=lambda i: -dims[i][0])

    def digest(size, row):
        group = []
        while rest and R.bit_ceil(dims[rest[0]][0]) == size:
            group.append(rest.pop(0))
        if not group:
            return None
        if row >= dims[group[0]][0]:
            assert all(not np.asarray(opened[i]).any() for i in group)
            return np.zeros((1, 8), dtype=np.uint64)
        return R.hash_rows(np.concatenate([np.asarray(opened[i], dtype=np.uint64) for i in group])[None, :], external)

    size = R.bit_ceil(dims[rest[0]][0])
    cur = digest(size, index)
    for sib in siblings:
        sib = np.asarray(sib, dtype=np.uint64)[None, :]
        cur = R.compress(cur, sib, external) if index & 1 == 0 else R.compress(sib, cur, external)
        index >>= 1
        size >>= 1
        inject = digest(size, index)
        if inject is not None:
            cur = R.compress(cur, inject, external)
    return bool((cur[0] == np.asarray(root, dtype=np.uint64)).all())


@pytest.mark.parametrize("case", ["bit_reversed_32_32_8", "plain_24_6", "wide_32_4"])
def test_open_batch_equals_open(case):
    from tachyon_amd.poseidon2 import FieldMerkleTree
    if case == "plain_24_6":
        dims, flag = [(24, 3), (6, 2)], False
    elif case == "wide_32_4":
        dims, flag = [(32, 300), (4, 257)], True
    else:
        dims, flag = [(32, 5), (32, 33), (8, 1)], True
    mats = [rand_words(4400 + i, r * c).reshape(r, c) for i, (r, c) in enumerate(dims)]
    tree = FieldMerkleTree("horizen")
    assert tree.build([(stored(m), r, c) for m, (r, c) in zip(mats, dims)], bit_reversed=flag)
    root = canon(tree.root)
    layers = R.build(mats, "horizen", bit_reversed=flag)
    assert (root == layers[-1][0]).all()
    indices = batch_indices(32, 4401)
    got = tree.open_batch(indices)
    assert got is not None and len(got) == len(indices)
    for index, (rows, sibs) in zip(indices, got):
        assert (rows, sibs) == tree.open(index), index
        wrows, wsibs = R.open_at(mats, layers, index, bit_reversed=flag)
        assert rows == [stored(w) for w in wrows] and sibs == [stored(s) for s in wsibs], index
        if case == "plain_24_6" and index >= 24:
            assert all(r == bytes(len(r)) for r in rows)     # rows past the heights open as zeros
        assert verify_padded(root, dims, index, [canon(r) for r in rows], [canon(s) for s in sibs], "horizen"), index
        if index < min(r << (5 - R.ceil_log2(r)) for r, _ in dims):       # no padded row: poseidon2_ref's own walk
            assert R.verify(root, dims, index, [canon(r) for r in rows], [canon(s) for s in sibs], "horizen"), index

    # refusals: nothing is written
    from tachyon_amd._lib import lib
    fn = lib().tachyon_mi355x_baby_bear_merkle_tree_open_batch
    rows = [ctypes.create_string_buffer(b"\xaa" * (2 * c * 4), 2 * c * 4) for _, c in dims]
    ptrs = (ctypes.c_void_p * len(rows))(*[ctypes.addressof(r) for r in rows])
    sib = ctypes.create_string_buffer(b"\xaa" * (2 * 5 * 32), 2 * 5 * 32)
    ok = (ctypes.c_size_t * 2)(1, 31)
    bad = (ctypes.c_size_t * 2)(1, 32)
    assert fn(tree._h, ok, 0, ptrs, sib) == 0 and fn(tree._h, bad, 2, ptrs, sib) == 0
    assert fn(tree._h, None, 2, ptrs, sib) == 0 and fn(tree._h, ok, 2, None, sib) == 0
    assert fn(tree._h, ok, 2, ptrs, None) == 0 and fn(None, ok, 2, ptrs, sib) == 0
    assert fn(tree._h, ok, (1 << 16) + 1, ptrs, sib) == 0
    assert all(r.raw == b"\xaa" * len(r.raw) for r in rows) and sib.raw == b"\xaa" * len(sib.raw)
    assert fn(tree._h, ok, 2, ptrs, sib) == 1
    assert FieldMerkleTree("horizen").open_batch([0]) is None            # no tree built
    tree.close()


# ---- 4. answer_queries against answer_query
SHAPES = [((3,),), ((1, 2),), ((4, 2), (4, 2)), ((2,), (3, 3)), ((3, 3), (2, 2)), ((0,),)]
ALPHA = F.ext(1234567, 7654321, 1111111, 2013265920)
ZETA = F.ext(987654321, 5, 2013265920, 42)


def ended_opening(shape, log_blowup):
    """An opening of random matrices of 5 columns, one point each, taken to the
    end of its commit phase, and fri_ref's answer_query for the same inputs."""
    from tachyon_amd.fri import FriOpening
    fri = FriOpening(log_blowup)
    assert fri.begin(F.to_bytes(ALPHA))
    rounds = []
    for r, degs in enumerate(shape):
        mats = [rand_words(4500 + 10 * r + m, (5 << (d + log_blowup))).reshape(-1, 5) for m, d in enumerate(degs)]
        rounds.append((mats, [[ZETA]] * len(mats)))
        assert fri.add_round([(stored(m), m.shape[0], 5) for m in mats], [[F.to_bytes(ZETA)]] * len(mats)) is not None
    assert fri.answer_queries([0]) is None                   # before the phase has ended
    k = iter(range(100))
    roots = fri.commit_phase(lambda root: F.to_bytes(F.ext(3 + next(k), 5, 7, 11)))
    _, ro = F.reduce_openings(ALPHA, rounds, log_blowup)
    k = iter(range(100))
    want_roots, trees, vectors, _ = F.commit_phase([ro[lg] for lg in sorted(ro, reverse=True)], log_blowup,
                                                   lambda root: F.ext(3 + next(k), 5, 7, 11))
    assert roots == [stored(r) for r in want_roots]

    def want(index):
        return [(F.to_bytes(val), [stored(s) for s in sibs]) for val, sibs in F.answer_query(index, trees, vectors)]

    return fri, want


@pytest.mark.parametrize("log_blowup", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "_".join("".join(map(str, r)) for r in s))
def test_answer_queries_equals_answer_query(shape, log_blowup):
    fri, want = ended_opening(shape, log_blowup)
    n = 1 << fri.input_log_size(0)
    indices = batch_indices(n, 4501)
    got = fri.answer_queries(indices)
    assert got is not None and len(got) == len(indices)
    if fri.num_commits:
        assert fri.last_launches == 1                        # one launch for every query and tree
    for index, ans in zip(indices, got):
        assert ans == fri.answer_query(index), index
        assert ans == want(index), index
    assert fri.answer_queries([]) is None and fri.answer_queries([0, n]) is None
    assert fri.answer_queries(list(range(n)) * ((1 << 16) // n) + [0]) is None      # above 2^16
    fri.close()


# ---- 5. the whole proof
PROOF_CASES = {
    "3": dict(shape=((3,),), cols=((5,),), log_blowup=1, external="plonky3", queries=10, bits=8, points=((1,),)),
    "42_42": dict(shape=((4, 2), (4, 2)), cols=((5, 5), (5, 5)), log_blowup=1, external="plonky3", queries=10, bits=8,
                  points=((1, 1), (1, 1))),
    "533_4": dict(shape=((5, 3, 3), (4,)), cols=((5, 33, 1), (7,)), log_blowup=2, external="horizen", queries=33,
                  bits=12, points=((2, 1, 0), (1,))),
}


class Setup:
    """Commit on the device, the transcript up to the opening points, and the
    proof fri_ref alone makes of it."""

    def __init__(self, case, seed=4600):
        from tachyon_amd.poseidon2 import FieldMerkleTree
        c = PROOF_CASES[case]
        self.c = c
        lb, ext = c["log_blowup"], c["external"]
        self.ldes = [[B.coset_lde(rand_words(seed + 10 * r + m, (1 << d) * w).reshape(1 << d, w), lb, 31)
                      for m, (d, w) in enumerate(zip(degs, ws))] for r, (degs, ws) in enumerate(zip(c["shape"], c["cols"]))]
        self.devs = [[DeviceWords(stored(m)) for m in mats] for mats in self.ldes]
        self.trees = []
        for mats, ds in zip(self.ldes, self.devs):
            t = FieldMerkleTree(ext)
            assert t.build_ptr([(d.ptr, m.shape[0], m.shape[1]) for d, m in zip(ds, mats)], bit_reversed=True)
            self.trees.append(t)
        self.commits = [canon(t.root) for t in self.trees]
        self.layers = [R.build(mats, ext, bit_reversed=True) for mats in self.ldes]
        for commit, layers in zip(self.commits, self.layers):
            assert (commit == layers[-1][0]).all()
        ch, ref = pair(ext)
        for commit in self.commits:
            observe_both(ch, ref, commit)
        zetas = [ref.sample_ext(), ref.sample_ext()]
        assert canon(ch.sample_ext() + ch.sample_ext()).tolist() == np.concatenate(zetas).tolist()
        self.points = [[zetas[:n] for n in ns] for ns in c["points"]]
        self.ch_start, self.ref_start = ch, ref

        # fri_ref's proof
        ref = self.ref_start.clone()
        self.alpha = ref.sample_ext()
        rounds = [(mats, pts) for mats, pts in zip(self.ldes, self.points)]
        self.opened, ro = F.reduce_openings(self.alpha, rounds, lb)
        self.log_max = max(ro)
        inputs = [ro[lg] for lg in sorted(ro, reverse=True)]
        self.betas = []

        def on_commit(root):
            ref.observe(root)
            self.betas.append(ref.sample_ext())
            return self.betas[-1]

        self.roots, self.fri_trees, self.vectors, final = F.commit_phase(inputs, lb, on_commit, ext)
        self.final_eval = final[0]
        ref.observe(self.final_eval)
        self.witness = ref.grind(c["bits"])
        self.indices = [ref.sample_bits(self.log_max) for _ in range(c["queries"])]
        self.ref_end = ref

    def rounds_arg(self):
        return [(t, [[F.to_bytes(z) for z in ps] for ps in pts]) for t, pts in zip(self.trees, self.points)]

    def prove(self, fri, ch):
        c = self.c
        return fri.prove(ch, self.rounds_arg(), c["queries"], c["bits"])

    def check(self, proof, opened):
        """every part of the proof bytewise against fri_ref's"""
        for r, per_round in enumerate(self.opened):
            for m, per_matrix in enumerate(per_round):
                assert opened[r][m] == [F.to_bytes(y) for y in per_matrix], (r, m)
        assert proof.commit_phase_commits == [stored(r) for r in self.roots]
        assert proof.final_eval == F.to_bytes(self.final_eval)
        assert proof.pow_witness == mont(self.witness)
        assert proof.num_queries == len(self.indices)
        for q, index in enumerate(self.indices):
            assert proof.query_index(q) == index
            want = F.answer_query(index, self.fri_trees, self.vectors)
            got = proof.query_steps(q)
            assert len(got) == len(want)
            for (val, sibs), (wval, wsibs) in zip(got, want):
                assert val == F.to_bytes(wval) and sibs == [stored(s) for s in wsibs], q
            for r, (mats, layers) in enumerate(zip(self.ldes, self.layers)):
                shifted = index >> (self.log_max - (len(layers) - 1))
                wrows, wsibs = R.open_at(mats, layers, shifted, bit_reversed=True)
                rows, sibs = proof.query_input(q, r)
                assert rows == [stored(w) for w in wrows] and sibs == [stored(s) for s in wsibs], (q, r)

    def as_tuple(self, proof):
        return (proof.commit_phase_commits, proof.final_eval, proof.pow_witness,
                [(proof.query_index(q), proof.query_steps(q), [proof.query_input(q, r) for r in range(len(self.trees))])
                 for q in range(proof.num_queries)])

    def verify(self, proof, opened, tamper=None) -> bool:
        """fri::Verify and VerifyOpeningProof's callback from a fresh challenger,
        on the proof's own bytes.  tamper(q, steps) may change a query's steps."""
        c = self.c
        ext, lb = c["external"], c["log_blowup"]
        v = self.ref_start.clone()
        alpha = v.sample_ext()
        roots = [canon(r) for r in proof.commit_phase_commits]
        if len(roots) != self.log_max - lb:
            return False
        betas = []
        for root in roots:
            v.observe(root)
            betas.append(v.sample_ext())
        final_eval = F.from_bytes(proof.final_eval)[0]
        v.observe(final_eval)
        if not v.check_witness(c["bits"], int(R.from_mont_words([proof.pow_witness])[0])):
            return False
        for q in range(proof.num_queries):
            index = v.sample_bits(self.log_max)
            if index != proof.query_index(q):
                return False
            rounds = []
            for r, (mats, commit, pts) in enumerate(zip(self.ldes, self.commits, self.points)):
                rows, sibs = proof.query_input(q, r)
                rows, sibs = [canon(x) for x in rows], [canon(s) for s in sibs]
                log_round = max(m.shape[0] for m in mats).bit_length() - 1
                dims = [m.shape for m in mats]
                if not R.verify(commit, dims, index >> (self.log_max - log_round), rows, sibs, ext):
                    return False
                rounds.append([(m.shape[0].bit_length() - 1, zs, [F.from_bytes(y) for y in ys], row)
                               for m, zs, ys, row in zip(mats, pts, opened[r], rows)])
            steps = [(F.from_bytes(val)[0], [canon(s) for s in sibs]) for val, sibs in proof.query_steps(q)]
            if tamper:
                tamper(q, steps)
            reduced = F.verifier_reduced_openings(index, self.log_max, alpha, rounds)
            folded = F.verify_query(index, self.log_max, betas, roots, steps, reduced, ext)
            if folded is None or not (folded == final_eval).all():
                return False
        return True

    def close(self):
        for t in self.trees:
            t.close()


@pytest.mark.parametrize("case", list(PROOF_CASES))
def test_prove_bytewise_and_verified(case):
    from tachyon_amd.fri import FriOpening
    s = Setup(case)
    fri = FriOpening(s.c["log_blowup"], s.c["external"])
    ch = s.ch_start.clone()
    result = s.prove(fri, ch)
    assert result is not None
    proof, opened = result
    s.check(proof, opened)
    assert s.verify(proof, opened)

    def flip(q, steps):
        if q == 1:
            steps[0][1][0] = steps[0][1][0].copy()
            steps[0][1][0][3] = (steps[0][1][0][3] + np.uint64(1)) % np.uint64(P)

    assert not s.verify(proof, opened, tamper=flip)
    # the transcript can go on
    assert same_state(ch, s.ref_end)
    assert int(canon(ch.sample())[0]) == s.ref_end.clone().sample()
    # the step API still answers on the same handle, and agrees
    assert fri.answer_query(s.indices[0]) == proof.query_steps(0)
    proof.close()
    fri.close()
    s.close()


# ---- 6. refusals of prove
def test_prove_refusals():
    from tachyon_amd._lib import FriRound, lib
    from tachyon_amd.fri import DuplexChallenger, FriOpening
    from tachyon_amd.poseidon2 import FieldMerkleTree
    L = lib()
    s = Setup("3")
    c = s.c
    fri = FriOpening(c["log_blowup"], c["external"])
    ch = s.ch_start.clone()
    first, opened = s.prove(fri, ch)
    s.check(first, opened)
    want = s.as_tuple(first)
    good = s.rounds_arg()
    tree, pts = good[0]
    lde = s.ldes[0][0]

    plain = FieldMerkleTree(c["external"])                     # built without the flag
    assert plain.build_ptr([(s.devs[0][0].ptr, lde.shape[0], lde.shape[1])], bit_reversed=False)
    plain._cols = tree._cols
    other = FieldMerkleTree("horizen")                         # another external matrix than the opening's
    assert other.build_ptr([(s.devs[0][0].ptr, lde.shape[0], lde.shape[1])], bit_reversed=True)
    unbuilt = FieldMerkleTree(c["external"])
    unbuilt._cols = tree._cols
    short = FieldMerkleTree(c["external"])                     # one row: below 2^log_blowup, which add_round refuses
    assert short.build_ptr([(s.devs[0][0].ptr, 1, lde.shape[1])], bit_reversed=True)
    wrong_ch = DuplexChallenger("horizen", 8)
    on_coset = F.to_bytes(F.from_base(np.uint64(F.coset_points(lde.shape[0])[5])))

    def attempts():
        q, b = c["queries"], c["bits"]
        yield "no rounds", lambda ch: fri.prove(ch, [], q, b)
        yield "no queries", lambda ch: fri.prove(ch, good, 0, b)
        yield "too many queries", lambda ch: fri.prove(ch, good, (1 << 16) + 1, b)
        yield "31 bits", lambda ch: fri.prove(ch, good, q, 31)
        yield "tree not built", lambda ch: fri.prove(ch, [(unbuilt, pts)], q, b)
        yield "tree without the flag", lambda ch: fri.prove(ch, [(plain, pts)], q, b)
        yield "tree of another matrix", lambda ch: fri.prove(ch, [(other, pts)], q, b)
        yield "challenger of another matrix", lambda ch: fri.prove(wrong_ch, good, q, b)
        yield "rows below the blowup", lambda ch: fri.prove(ch, [(short, pts)], q, b)
        yield "a non-canonical point", lambda ch: fri.prove(ch, [(tree, [[b"\xff" * 16]])], q, b)
        yield "a second round that is refused", lambda ch: fri.prove(ch, good + [(unbuilt, pts)], q, b)
        rec = (FriRound * 1)()
        keep = []

        def raw(ch, tree_h=tree._h, points=True, nums=True, outs=True, h=fri._h, rounds=True, challenger=True):
            pbuf = ctypes.create_string_buffer(F.to_bytes(s.points[0][0][0]), 16)
            obuf = ctypes.create_string_buffer(16 * lde.shape[1])
            pp = (ctypes.c_void_p * 1)(ctypes.addressof(pbuf))
            np_ = (ctypes.c_size_t * 1)(1)
            op = (ctypes.c_void_p * 1)(ctypes.addressof(obuf))
            keep.append((pbuf, obuf, pp, np_, op))
            rec[0] = FriRound(tree_h, pp if points else None, np_ if nums else None, op if outs else None)
            return L.tachyon_mi355x_baby_bear_fri_opening_prove(h, ch._h if challenger else None, rec if rounds else None,
                                                                 1, q, b) or None

        yield "null opening", lambda ch: raw(ch, h=None)
        yield "null challenger", lambda ch: raw(ch, challenger=False)
        yield "null rounds", lambda ch: raw(ch, rounds=False)
        yield "null tree", lambda ch: raw(ch, tree_h=None)
        yield "null points", lambda ch: raw(ch, points=False)
        yield "null num_points", lambda ch: raw(ch, nums=False)
        yield "null outputs", lambda ch: raw(ch, outs=False)

    for name, attempt in attempts():
        ch = s.ch_start.clone()
        before = ch.state()
        step_before = fri.answer_query(s.indices[0])
        assert attempt(ch) is None, name
        assert ch.state() == before, name                     # the challenger is as it was
        assert fri.answer_query(s.indices[0]) == step_before, name   # and so is the opening
        again, opened = s.prove(fri, ch)                       # the same handles produce the correct proof
        assert s.as_tuple(again) == want, name
        again.close()

    # a point inside the coset: the challenger is restored, the opening needs a new begin
    ch = s.ch_start.clone()
    before = ch.state()
    assert fri.prove(ch, [(tree, [[on_coset]])], c["queries"], c["bits"]) is None
    assert ch.state() == before and fri.answer_query(0) is None and fri.commit() is None
    again, opened = s.prove(fri, ch)
    assert s.as_tuple(again) == want
    for t in (plain, other, unbuilt, short):
        t.close()
    fri.close()
    s.close()


# ---- 7. elements at any 4-byte alignment
def test_extension_elements_need_no_16_byte_alignment():
    """A C or C++ caller keeps alpha, beta and the points in std::array<F, 4> on
    its stack, aligned to 4 bytes: the step API and prove give the same bytes
    for elements at offsets 4, 8 and 12 of a 16-byte-aligned buffer as for
    aligned ones."""
    from tachyon_amd._lib import FriRound, lib
    from tachyon_amd.fri import FriOpening
    L = lib()
    s = Setup("3")
    c = s.c
    lde, dev = s.ldes[0][0], s.devs[0][0]
    fri = FriOpening(c["log_blowup"], c["external"])
    ch = s.ch_start.clone()
    first, opened = s.prove(fri, ch)
    s.check(first, opened)
    want = s.as_tuple(first)
    zeta, alpha = F.to_bytes(s.points[0][0][0]), F.to_bytes(s.alpha)
    for off in (4, 8, 12):
        raw = ctypes.create_string_buffer(64 + 16)
        base = (ctypes.addressof(raw) + 15) // 16 * 16 + off

        def at(data):
            ctypes.memmove(base, data, 16)
            return base

        # prove with a point at the offset
        obuf = ctypes.create_string_buffer(16 * lde.shape[1])
        pp, nums = (ctypes.c_void_p * 1)(at(zeta)), (ctypes.c_size_t * 1)(1)
        op = (ctypes.c_void_p * 1)(ctypes.addressof(obuf))
        rec = (FriRound * 1)(FriRound(s.trees[0]._h, pp, nums, op))
        ch = s.ch_start.clone()
        h = L.tachyon_mi355x_baby_bear_fri_opening_prove(fri._h, ch._h, rec, 1, c["queries"], c["bits"])
        assert h, off
        L.tachyon_mi355x_baby_bear_fri_proof_destroy(h)
        assert obuf.raw == opened[0][0][0], off
        # the step API: alpha, the point and every beta at the offset
        assert L.tachyon_mi355x_baby_bear_fri_opening_begin(fri._h, at(alpha)) == 1
        one = (ctypes.c_size_t * 1)
        mat = (ctypes.c_void_p * 1)(dev.ptr)
        pp = (ctypes.c_void_p * 1)(at(zeta))
        assert L.tachyon_mi355x_baby_bear_fri_opening_add_round(fri._h, mat, one(lde.shape[0]), one(lde.shape[1]), 1,
                                                                pp, one(1), op) == 1
        assert obuf.raw == opened[0][0][0], off
        betas = iter(s.betas)
        roots = []
        root = ctypes.create_string_buffer(32)
        while L.tachyon_mi355x_baby_bear_fri_opening_commit(fri._h, root) == 1:
            roots.append(root.raw)
            assert L.tachyon_mi355x_baby_bear_fri_opening_fold(fri._h, at(F.to_bytes(next(betas)))) == 1
        assert roots == want[0] and fri.final_eval == want[1], off
    first.close()
    fri.close()
    s.close()


# ---- 8. the C++ client
@pytest.mark.parametrize("external", EXTERNALS)
def test_cpp_client_prove(external):
    """bin/baby_bear_fri_prove_check: Commit, FriOpening::Prove with a
    DuplexChallenger through the header, checked inside the program against the
    step API and a replayed transcript"""
    exe = os.path.join(BIN, "baby_bear_fri_prove_check")
    assert os.path.exists(exe), "bin/baby_bear_fri_prove_check is built by build()"
    log_rows, cols, queries, bits = 8, 7, 12, 10
    gen = B.mont(B.root_of_unity(2 << log_rows))
    r = subprocess.run([exe, "--external", external, "--gen", str(gen), str(log_rows), str(cols), str(queries), str(bits)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout)
    assert got["ok"] is True and got["commits"] == log_rows and got["queries"] == queries


# ---- 9. a single index is a batch of one
def test_answer_query_is_answer_queries_at_one_index():
    """log_blowup 1, inputs at log heights 5 and 3: the first, an inner and the
    last index against fri_ref, one launch each; the first index out of range is
    refused by both calls, which leave the caller's buffers alone"""
    from tachyon_amd._lib import lib
    fri, want = ended_opening(((4, 2),), 1)
    assert fri.input_log_size(0) == 5 and fri.input_log_size(1) == 3 and fri.num_commits == 4
    for index in (0, 13, 31):
        single = fri.answer_query(index)
        assert fri.last_launches == 1
        assert single == want(index), index
        batch = fri.answer_queries([index])
        assert fri.last_launches == 1
        assert batch == [single], index
    assert fri.answer_query(32) is None and fri.answer_queries([32]) is None
    vals = ctypes.create_string_buffer(b"\xaa" * (4 * 16), 4 * 16)
    sibs = ctypes.create_string_buffer(b"\xaa" * (10 * 32), 10 * 32)           # 4 + 3 + 2 + 1 digests
    idx = (ctypes.c_size_t * 1)(32)
    assert lib().tachyon_mi355x_baby_bear_fri_opening_answer_query(fri._h, 32, vals, sibs) == 0
    assert lib().tachyon_mi355x_baby_bear_fri_opening_answer_queries(fri._h, idx, 1, vals, sibs) == 0
    assert vals.raw == b"\xaa" * len(vals.raw) and sibs.raw == b"\xaa" * len(sibs.raw)
    assert lib().tachyon_mi355x_baby_bear_fri_opening_answer_query(fri._h, 31, vals, sibs) == 1
    assert _split(vals.raw, sibs.raw, 5, 4) == want(31)
    fri.close()


def _split(vals: bytes, sibs: bytes, log_max: int, commits: int):
    out, at = [], 0
    for i in range(commits):
        n = log_max - i - 1
        out.append((vals[16 * i:16 * (i + 1)], [sibs[32 * (at + k):32 * (at + k + 1)] for k in range(n)]))
        at += n
    return out


@pytest.mark.parametrize("log_blowup", [1, 2])
def test_answer_query_without_a_commit_phase_tree(log_blowup):
    """The largest input has log height log_blowup: nothing is committed.  The
    single call answers without looking at its output pointers; the batched one
    wants its first array, and neither writes."""
    from tachyon_amd._lib import lib
    L = lib()
    fri, want = ended_opening(((0,),), log_blowup)
    n = 1 << log_blowup
    assert fri.num_commits == 0 and fri.input_log_size(0) == log_blowup
    buf = ctypes.create_string_buffer(b"\xaa" * 64, 64)
    idx = (ctypes.c_size_t * 2)(n - 1, 0)
    assert L.tachyon_mi355x_baby_bear_fri_opening_answer_query(fri._h, n - 1, None, None) == 1
    assert L.tachyon_mi355x_baby_bear_fri_opening_answer_query(fri._h, n - 1, buf, None) == 1
    assert L.tachyon_mi355x_baby_bear_fri_opening_answer_query(fri._h, n, None, None) == 0
    assert L.tachyon_mi355x_baby_bear_fri_opening_answer_queries(fri._h, idx, 2, buf, None) == 1
    assert L.tachyon_mi355x_baby_bear_fri_opening_answer_queries(fri._h, idx, 2, None, None) == 0
    idx[1] = n
    assert L.tachyon_mi355x_baby_bear_fri_opening_answer_queries(fri._h, idx, 2, buf, None) == 0
    assert buf.raw == b"\xaa" * 64
    assert fri.answer_query(n - 1) == [] == want(n - 1) and fri.answer_queries([0, n - 1]) == [[], []]
    assert fri.answer_query(n) is None and fri.answer_queries([n]) is None
    fri.close()


# A tree takes no two heights that round up to the same power of two, and the
# bit-reversed flag takes powers of two only, so the 32-row matrices and the
# 30-row one cannot share a tree: the 30-row matrix stands with a short one.
ONE_INDEX_TREES = {"natural_32_32": ([(32, 5), (32, 3)], False), "bit_reversed_32_32": ([(32, 5), (32, 3)], True),
                   "natural_30_4": ([(30, 7), (4, 2)], False)}


@pytest.mark.parametrize("case", list(ONE_INDEX_TREES))
def test_open_is_open_batch_at_one_index(case):
    from tachyon_amd.poseidon2 import FieldMerkleTree
    dims, flag = ONE_INDEX_TREES[case]
    mats = [rand_words(4700 + i, r * c).reshape(r, c) for i, (r, c) in enumerate(dims)]
    tree = FieldMerkleTree("horizen")
    assert tree.build([(stored(m), r, c) for m, (r, c) in zip(mats, dims)], bit_reversed=flag)
    launches = tree.last_launches
    layers = R.build(mats, "horizen", bit_reversed=flag)
    assert (canon(tree.root) == layers[-1][0]).all()
    for index in (0, 29, 30, 31):
        wrows, wsibs = R.open_at(mats, layers, index, bit_reversed=flag)
        want = ([stored(w) for w in wrows], [stored(s) for s in wsibs])
        assert tree.open(index) == want, index
        assert tree.open_batch([index]) == [want], index
        assert tree.last_launches == launches
        if dims[0][0] == 30 and index >= 30:                 # past 30 rows: zeros; row 3 of 4 is there
            assert want[0][0] == bytes(4 * 7) and want[0][1] != bytes(4 * 2)
    assert tree.open(32) is None and tree.open_batch([32]) is None
    if not flag:                                             # what keeps 32 and 30 rows out of one tree
        both = [(32, 5), (30, 7)]
        assert not tree.build([(bytes(4 * r * c), r, c) for r, c in both])
        assert not tree.build([(bytes(4 * 30 * 7), 30, 7)], bit_reversed=True)
        assert tree.open(31) == want                         # a refused build leaves the tree as it was
    tree.close()


def test_open_on_a_one_leaf_tree():
    """one matrix of one row: the root is the leaf's hash, there are no
    siblings, and open wants no siblings_out"""
    from tachyon_amd._lib import lib
    from tachyon_amd.poseidon2 import FieldMerkleTree
    L = lib()
    mat = rand_words(4800, 6).reshape(1, 6)
    tree = FieldMerkleTree("horizen")
    assert tree.build([(stored(mat), 1, 6)])
    launches = tree.last_launches
    layers = R.build([mat], "horizen")
    assert len(layers) == 1 and (canon(tree.root) == layers[0][0]).all()
    row = ctypes.create_string_buffer(b"\xaa" * 24, 24)
    ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(row))
    idx = (ctypes.c_size_t * 1)(0)
    assert L.tachyon_mi355x_baby_bear_merkle_tree_open(tree._h, 0, ptrs, None) == 1 and row.raw == stored(mat)
    row.raw = b"\xaa" * 24
    assert L.tachyon_mi355x_baby_bear_merkle_tree_open_batch(tree._h, idx, 1, ptrs, None) == 1
    assert row.raw == stored(mat)
    row.raw = b"\xaa" * 24
    idx[0] = 1
    assert L.tachyon_mi355x_baby_bear_merkle_tree_open(tree._h, 1, ptrs, None) == 0
    assert L.tachyon_mi355x_baby_bear_merkle_tree_open_batch(tree._h, idx, 1, ptrs, None) == 0
    assert row.raw == b"\xaa" * 24
    assert tree.open(0) == ([stored(mat)], []) == tree.open_batch([0])[0] and tree.open(1) is None
    assert tree.last_launches == launches
    tree.close()
