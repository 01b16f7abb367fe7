"""BabyBear4 and the FRI opening on the GPU at the boundary (tachyon_amd.fri
over tachyon_mi355x_baby_bear4_ops / tachyon_mi355x_baby_bear_fri_opening_*),
compared bytewise with tests/fri_ref.py: the field at its operand bounds, the
opened values and reduced openings, the fold steps, every commit-phase root,
the queries, the refusals, the C++ client bin/baby_bear_fri_check, and a full
protocol run driven by fri_ref's challenger and checked by its verifier walk.

Inputs are default_rng(seed) words in [0, p); every case also runs with all
words p - 1 and with a single non-zero word.  Device matrices sit between guard
bands of sentinel words.  There are no tolerances: every result is a canonical
field element.

Sizes at which the launch plan changes path, all covered below:
  columns staged per tile of the rr pass   cols 31|32|33, 64|65 (a last tile that is full, short, one word)
  positions per block of the rr pass       n = 2 .. 256 (part of one block), 512 and more (several blocks)
  points per interpolation launch          1, 2, 3|4, 5|8 (template sizes), 9 (a second group)
  64 columns per interpolation block       cols 64|65, 67, 300
  rows per interpolation block             below 128 one short block; log degree 13: two tiles of 64 rows per block
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
KINDS = ["random", "pm1", "single"]
SENTINEL = 0x5EA7BEEF
GUARD = 1024           # sentinel words before and after a device buffer
ALPHA = F.ext(1234567, 7654321, 1111111, 2013265920)
ZETA = F.ext(987654321, 5, 2013265920, 42)          # the point shared across matrices and rounds


def words(kind: str, seed: int, count: int) -> np.ndarray:
    """canonical words"""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, P, size=count, dtype=np.uint64)
    if kind == "pm1":
        return np.full(count, P - 1, dtype=np.uint64)
    w = np.zeros(count, dtype=np.uint64)
    w[(seed * 7919) % count] = 1 + seed % (P - 1)
    return w


def stored(x) -> bytes:
    return R.to_bytes(R.mont_words(np.asarray(x, dtype=np.uint64).reshape(-1)))


class DeviceWords:
    """Words on the device between two guard bands of sentinel words."""

    def __init__(self, data: bytes):
        import torch
        self.n = len(data) // 4
        host = np.full(self.n + 2 * GUARD, SENTINEL, dtype=np.uint32)
        host[GUARD:GUARD + self.n] = np.frombuffer(data, dtype="<u4")
        self.t = torch.from_numpy(host.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + 4 * GUARD

    def read(self) -> bytes:
        import torch
        torch.cuda.synchronize()
        raw = self.t.cpu().numpy().view(np.uint32)
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + self.n:] == SENTINEL).all(), "guard band written"
        return raw[GUARD:GUARD + self.n].astype("<u4").tobytes()


def points_for(seed: int, count: int):
    """`count` points: the shared one first, then seeded ones"""
    rng = np.random.default_rng(seed)
    return [ZETA] + [rng.integers(0, P, size=4, dtype=np.uint64) for _ in range(count - 1)] if count else []


def make_rounds(kind, seed, log_degrees_by_round, cols, log_blowup, num_points):
    """(mats, points) per round in fri_ref's form: natural-order (n, cols) arrays"""
    rounds = []
    for r, degs in enumerate(log_degrees_by_round):
        mats, pts = [], []
        for m, d in enumerate(degs):
            n = 1 << (d + log_blowup)
            s = seed + 100 * r + m
            mats.append(words(kind, s, n * cols).reshape(n, cols))
            pts.append(points_for(s, num_points))
        rounds.append((mats, pts))
    return rounds


def run_reduce(fri, rounds, device=True):
    """begin + every round on the GPU; returns (opened values, device buffers)"""
    assert fri.begin(F.to_bytes(ALPHA))
    devs, out = [], []
    for mats, pts in rounds:
        zs = [[F.to_bytes(z) for z in ps] for ps in pts]
        if device:
            ds = [DeviceWords(stored(m)) for m in mats]
            devs += ds
            ys = fri.add_round_ptr([(d.ptr, m.shape[0], m.shape[1]) for d, m in zip(ds, mats)], zs)
        else:
            ys = fri.add_round([(stored(m), m.shape[0], m.shape[1]) for m in mats], zs)
        assert ys is not None
        out.append(ys)
    return out, devs


def check_reduce(fri, rounds, log_blowup, device=True):
    """opened values and every reduced opening against fri_ref; returns fri_ref's inputs, largest first"""
    want_opened, want_ro = F.reduce_openings(ALPHA, rounds, log_blowup)
    got, devs = run_reduce(fri, rounds, device)
    for r, (mats, pts) in enumerate(rounds):
        for m in range(len(mats)):
            assert len(got[r][m]) == len(pts[m])
            for p in range(len(pts[m])):
                assert got[r][m][p] == F.to_bytes(want_opened[r][m][p]), (r, m, p)
    logs = sorted(want_ro, reverse=True)
    assert fri.num_inputs == len(logs)
    for k, lg in enumerate(logs):
        assert fri.input_log_size(k) == lg
        assert fri.input(k) == F.to_bytes(want_ro[lg]), f"reduced opening 2^{lg}"
    for d, m in zip(devs, [m for mats, _ in rounds for m in mats]):
        assert d.read() == stored(m)            # the matrices are untouched, the guard bands too
    return [want_ro[lg] for lg in logs]


def betas():
    k = 0
    while True:
        yield F.ext(3 + k, P - 1 - k, 77 * k + 1, 123456789)
        k += 1


def check_commit_phase(fri, inputs, log_blowup, external, indices):
    """roots, the final values and answer_query at `indices` against fri_ref"""
    bs = betas()
    roots, trees, vectors, final = F.commit_phase(inputs, log_blowup, lambda root: next(bs), external)
    bs = betas()
    seen = []
    got = fri.commit_phase(lambda root: (seen.append(root), F.to_bytes(next(bs)))[1])
    assert got == seen == [stored(r) for r in roots]
    assert fri.num_commits == len(roots)
    assert fri.final_poly() == F.to_bytes(final)
    assert fri.final_eval == F.to_bytes(final[0])
    assert fri.commit() is None                       # the phase has ended
    for index in indices:
        want = F.answer_query(index, trees, vectors)
        ans = fri.answer_query(index)
        assert ans is not None and len(ans) == len(want)
        for (val, sibs), (wval, wsibs) in zip(ans, want):
            assert val == F.to_bytes(wval), index
            assert sibs == [stored(s) for s in wsibs], index
    return final


# ---- 1. the field on the device at its operand bounds
def ext_operands(kind, seed, count):
    a = words(kind, seed, 4 * count).reshape(count, 4)
    b = words(kind, seed + 1, 4 * count).reshape(count, 4)
    return a, b


REF_OPS = {"add": F.e_add, "sub": F.e_sub, "mul": F.e_mul, "square": lambda a, b: F.e_mul(a, a),
           "inverse": lambda a, b: F.e_inv(a)}


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("op", list(REF_OPS))
def test_baby_bear4_ops(op, count):
    from tachyon_amd.fri import baby_bear4_ops, baby_bear4_ops_ptr
    for kind in KINDS:
        a, b = ext_operands(kind, 9100 + count, count)
        want = F.to_bytes(REF_OPS[op](a, b))
        unary = op in ("square", "inverse")
        assert baby_bear4_ops(op, F.to_bytes(a), None if unary else F.to_bytes(b)) == want, (op, kind)
        da, db, do = DeviceWords(F.to_bytes(a)), DeviceWords(F.to_bytes(b)), DeviceWords(bytes(16 * count))
        assert baby_bear4_ops_ptr(op, da.ptr, None if unary else db.ptr, do.ptr, count)
        assert do.read() == want, (op, kind)
        assert da.read() == F.to_bytes(a) and db.read() == F.to_bytes(b)


def test_baby_bear4_golden_and_refusals():
    from tachyon_amd.fri import baby_bear4_ops, baby_bear4_ops_ptr
    with open(os.path.join(ROOT, "tests", "golden", "fri_baby_bear.json")) as f:
        rec = json.load(f)["recorded"]
    a, b = np.array(rec["a"], dtype=np.uint64), np.array(rec["b"], dtype=np.uint64)
    assert baby_bear4_ops("mul", F.to_bytes(a), F.to_bytes(b)) == F.to_bytes(np.array(rec["product"]))
    assert baby_bear4_ops("inverse", F.to_bytes(a)) == F.to_bytes(np.array(rec["inverse_a"]))
    assert baby_bear4_ops("inverse", bytes(16)) == bytes(16)          # the inverse of 0 is 0
    buf = ctypes.create_string_buffer(64)
    d = DeviceWords(bytes(64))
    p = ctypes.addressof(buf)
    assert not baby_bear4_ops_ptr(5, p, p, p, 4) and not baby_bear4_ops_ptr(-1, p, p, p, 4)
    assert not baby_bear4_ops_ptr("mul", p, None, p, 4) and not baby_bear4_ops_ptr("mul", None, p, p, 4)
    assert not baby_bear4_ops_ptr("mul", p, p, None, 4) and not baby_bear4_ops_ptr("mul", p, p, p, 0)
    assert not baby_bear4_ops_ptr("mul", p, p, p, (1 << 28) + 1)
    assert not baby_bear4_ops_ptr("add", p, p, d.ptr, 4) and not baby_bear4_ops_ptr("add", d.ptr, p, d.ptr, 4)
    assert d.read() == bytes(64)


# ---- 2. reduced openings: the reference unit test's shapes
SHAPES = [((3,),), ((1, 2),), ((4, 2), (4, 2)), ((2,), (3, 3)), ((3, 3), (2, 2)), ((0,),)]


@pytest.mark.parametrize("num_points", [0, 1, 2, 5])
@pytest.mark.parametrize("log_blowup", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "_".join("".join(map(str, r)) for r in s))
def test_reduced_openings_reference_shapes(shape, log_blowup, num_points):
    from tachyon_amd.fri import FriOpening
    fri = FriOpening(log_blowup)
    for kind in KINDS:
        rounds = make_rounds(kind, 9300, shape, 5, log_blowup, num_points)
        check_reduce(fri, rounds, log_blowup)
    fri.close()


# ---- 3. reduced openings: the boundary shapes and every change of path
@pytest.mark.parametrize("cols", [1, 5, 31, 32, 33, 64, 65, 67, 300])
def test_reduced_openings_columns(cols):
    from tachyon_amd.fri import FriOpening
    fri = FriOpening(1)
    for kind in KINDS:
        check_reduce(fri, make_rounds(kind, 9400 + cols, ((6,),), cols, 1, 2), 1)
    fri.close()


@pytest.mark.parametrize("num_points", [3, 4, 8, 9])
def test_reduced_openings_point_groups(num_points):
    from tachyon_amd.fri import FriOpening
    fri = FriOpening(1)
    check_reduce(fri, make_rounds("random", 9500, ((6, 3),), 7, 1, num_points), 1)
    fri.close()


@pytest.mark.parametrize("cols", [67, 300])
def test_reduced_openings_log_degree_13(cols):
    """rows beyond one workgroup and one staging tile; an interpolation block
    covers two tiles of rows"""
    from tachyon_amd.fri import FriOpening
    fri = FriOpening(1)
    check_reduce(fri, make_rounds("random", 9600, ((13,),), cols, 1, 2), 1)
    # alpha powers, two inverse-denominator vectors, interpolate + finish + reduced ys for the group of two, the rr pass
    assert fri.last_launches == 1 + 2 + 3 + 1
    fri.close()


def test_reduced_openings_host_memory():
    from tachyon_amd.fri import FriOpening
    fri = FriOpening(2)
    check_reduce(fri, make_rounds("random", 9700, ((4, 2), (4, 2)), 5, 2, 2), 2, device=False)
    fri.close()


# ---- 4. fold steps, additions, roots, queries
@pytest.mark.parametrize("external", ["horizen", "plonky3"])
def test_commit_phase_from_2_14_through_the_tail(external):
    """2^14 down to 2 with inputs joining at 2^10 and 2^3, every root, and the
    queries at sampled indices of the largest input"""
    from tachyon_amd.fri import FriOpening
    fri = FriOpening(1, external)
    inputs = check_reduce(fri, make_rounds("random", 9800, ((13, 9, 2),), 3, 1, 1), 1)
    assert [i.shape[0] for i in inputs] == [1 << 14, 1 << 10, 1 << 3]
    assert fri.answer_query(0) is None                 # before the phase has ended
    check_commit_phase(fri, inputs, 1, external, [0, 1, 2, 8191, 8192, 12345, (1 << 14) - 1])
    assert fri.num_commits == 13 and fri.answer_query(1 << 14) is None
    fri.close()


@pytest.mark.parametrize("log_blowup", [1, 2])
def test_small_case_every_index_and_honest_final_values(log_blowup):
    """{{4,2},{4,2}} on honest extensions: the final values are all equal, and
    answer_query at every index shows every digest of every commit-phase layer
    (each one is some leaf's sibling) against poseidon2_ref.build"""
    from tachyon_amd.fri import FriOpening
    rounds = []
    for r in range(2):
        mats = [B.coset_lde(words("random", 9900 + 10 * r + m, (1 << d) * 5).reshape(1 << d, 5), log_blowup, 31)
                for m, d in enumerate((4, 2))]
        rounds.append((mats, [[ZETA], [ZETA, F.ext(9, 8, 7, 6)]]))
    fri = FriOpening(log_blowup)
    inputs = check_reduce(fri, rounds, log_blowup)
    final = check_commit_phase(fri, inputs, log_blowup, "horizen", range(1 << (4 + log_blowup)))
    assert (final == final[0]).all()
    # one corrupted row: no longer a low-degree extension
    rounds[0][0][0] = rounds[0][0][0].copy()
    rounds[0][0][0][3, 2] = (rounds[0][0][0][3, 2] + np.uint64(1)) % np.uint64(P)
    inputs = check_reduce(fri, rounds, log_blowup)
    final = check_commit_phase(fri, inputs, log_blowup, "horizen", [5])
    assert not (final == final[0]).all()
    fri.close()


def test_degree_zero_has_no_commit_phase():
    from tachyon_amd.fri import FriOpening
    fri = FriOpening(2)
    inputs = check_reduce(fri, make_rounds("random", 9950, ((0,),), 5, 2, 1), 2)
    assert fri.commit() is None and fri.num_commits == 0
    assert fri.final_poly() == F.to_bytes(inputs[0]) and fri.answer_query(3) == [] and fri.answer_query(4) is None
    fri.close()


# ---- 5. refusals
def test_refusals():
    from tachyon_amd._lib import lib
    from tachyon_amd.fri import FriOpening
    L = lib()
    for lb, ext_id in [(0, 0), (27, 0), (1, 2), (1, -1)]:
        assert not L.tachyon_mi355x_baby_bear_fri_opening_create(lb, ext_id, None)
    fri = FriOpening(2)
    good = make_rounds("random", 9960, ((3,),), 5, 2, 1)
    mat = good[0][0][0]
    data, z = stored(mat), [[F.to_bytes(ZETA)]]
    assert fri.add_round([(data, 32, 5)], z) is None          # before begin
    assert fri.commit() is None and not fri.fold(F.to_bytes(ALPHA)) and fri.final_poly() is None
    assert not fri.begin(b"\xff" * 16)                         # a non-canonical alpha
    assert fri.begin(F.to_bytes(ALPHA))
    assert fri.commit() is None                                # no input yet
    buf = ctypes.create_string_buffer(data)
    p = ctypes.addressof(buf)
    assert fri.add_round_ptr([(p, 32, 0)], z) is None          # no columns
    assert fri.add_round_ptr([(p, 24, 5)], z) is None          # rows no power of two
    assert fri.add_round_ptr([(p, 2, 5)], z) is None           # rows below 2^log_blowup
    assert fri.add_round_ptr([(p, 1 << 28, 5)], z) is None     # rows above 2^27
    assert fri.add_round_ptr([(None, 32, 5)], z) is None       # a null matrix
    assert fri.add_round_ptr([], []) is None                   # count 0
    assert fri.add_round_ptr([(p, 32, 5)], [[b"\xff" * 16]]) is None      # a non-canonical point
    one = (ctypes.c_size_t * 1)(1)
    ptr = (ctypes.c_void_p * 1)(p)
    add = L.tachyon_mi355x_baby_bear_fri_opening_add_round
    assert add(fri._h, None, one, one, 1, ptr, one, ptr) == 0 and add(fri._h, ptr, None, one, 1, ptr, one, ptr) == 0
    assert add(fri._h, ptr, one, None, 1, ptr, one, ptr) == 0 and add(fri._h, ptr, one, one, 1, None, one, ptr) == 0
    assert add(fri._h, ptr, one, one, 1, ptr, None, ptr) == 0 and add(fri._h, ptr, one, one, 1, ptr, one, None) == 0
    assert add(None, ptr, one, one, 1, ptr, one, ptr) == 0
    assert fri.num_inputs == 0                                 # the refusals left the handle as it was
    inputs = check_reduce(fri, good, 2)
    assert not fri.fold(F.to_bytes(ALPHA))                     # no pending commit
    assert fri.answer_query(0) is None
    root = fri.commit()
    assert root is not None and fri.commit() is None           # a root that fold has not consumed
    assert fri.add_round([(data, 32, 5)], z) is None           # the inputs are frozen
    assert fri.answer_query(0) is None and fri.final_poly() is None
    assert not fri.fold(b"\xff" * 16)
    assert fri.fold(F.to_bytes(ALPHA))
    assert fri.input(0) == F.to_bytes(inputs[0])

    # a point on the committed coset: x_5 of 31 <w_32>, found on the device
    on_coset = F.from_base(np.uint64(F.coset_points(32)[5]))
    assert F.reduce_openings(ALPHA, [([mat], [[on_coset]])], 2) is None
    assert fri.begin(F.to_bytes(ALPHA))
    assert fri.add_round([(data, 32, 5)], [[F.to_bytes(on_coset)]]) is None
    assert fri.add_round([(data, 32, 5)], z) is None and fri.commit() is None and fri.input(0) is None
    check_reduce(fri, good, 2)                                 # a new begin helps
    fri.close()


# ---- 6. the C++ client
def splitmix_words(seed: int, n: int) -> np.ndarray:
    """seeded() of check/baby_bear_fri_check.cc"""
    mask = (1 << 64) - 1
    out, x = np.empty(n, dtype=np.uint64), seed
    for i in range(n):
        x = (x + 0x9E3779B97F4A7C15) & mask
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        out[i] = z % P
    return out


def test_cpp_client_commit_then_open():
    exe = os.path.join(BIN, "baby_bear_fri_check")
    assert os.path.exists(exe), "bin/baby_bear_fri_check is built by build()"
    log_rows, cols, queries = 9, 7, 3
    gen = B.mont(B.root_of_unity(2 << log_rows))
    r = subprocess.run([exe, "--external", "plonky3", "--gen", str(gen), str(log_rows), str(cols), str(queries)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout)
    assert got["calls"] is True

    def canon(stored_words):
        return R.from_mont_words(np.array(stored_words, dtype=np.uint64))

    trace = R.from_mont_words(splitmix_words(0xF21F0000, (1 << log_rows) * cols)).reshape(-1, cols)
    lde = B.coset_lde(trace, 1, 31)
    assert (canon(got["commitment"]) == R.build([lde], "plonky3", bit_reversed=True)[-1][0]).all()
    alpha, zeta = canon([3, 1, 4, 1]), canon([5, 6, 7, 8])
    opened, ro = F.reduce_openings(alpha, [([lde], [[zeta]])], 1)
    assert (canon(got["opened_values"]) == opened[0][0][0]).all()
    step = iter(range(100))
    roots, trees, vectors, final = F.commit_phase([ro[log_rows + 1]], 1, lambda root: canon([next(step) + 2, 3, 4, 5]),
                                                  "plonky3")
    assert (canon(got["commit_phase_commits"]) == np.array(roots)).all()
    assert (canon(got["final_poly"]) == final).all() and (final == final[0]).all()
    for q, ans in enumerate(got["queries"]):
        assert ans["index"] == (q * 2654435761) % (2 << log_rows)
        want = F.answer_query(ans["index"], trees, vectors)
        assert len(ans["steps"]) == len(want)
        for s, (wval, wsibs) in zip(ans["steps"], want):
            assert (canon(s["sibling_value"]) == wval).all()
            assert (canon(s["opening_proof"]).reshape(-1, 8) == np.array(wsibs).reshape(-1, 8)).all()


# ---- 7. the whole protocol with a challenger, checked by the verifier walk
@pytest.mark.parametrize("shape", [((3,),), ((4, 2), (4, 2))], ids=["3", "42_42"])
def test_full_protocol_verifies(shape):
    """TwoAdicFRITest::TestProtocol: 5 columns, log_blowup 1, 10 queries, 8
    proof-of-work bits, Plonky3's external matrix, one point zeta everywhere.
    The prover is the GPU (trees, reduced openings, commit phase, queries) with
    fri_ref's DuplexChallenger as its transcript; the verifier is fri_ref."""
    from tachyon_amd.fri import FriOpening
    from tachyon_amd.poseidon2 import FieldMerkleTree
    external, log_blowup, cols, num_queries, pow_bits = "plonky3", 1, 5, 10, 8
    ldes = [[B.coset_lde(words("random", 9990 + 10 * r + m, (1 << d) * cols).reshape(1 << d, cols), log_blowup, 31)
             for m, d in enumerate(degs)] for r, degs in enumerate(shape)]
    # Commit: the round trees over the bit-reversed extensions, on the device
    devs = [[DeviceWords(stored(m)) for m in mats] for mats in ldes]
    round_trees = []
    for mats, ds in zip(ldes, devs):
        t = FieldMerkleTree(external)
        assert t.build_ptr([(d.ptr, m.shape[0], cols) for d, m in zip(ds, mats)], bit_reversed=True)
        round_trees.append(t)
    commits = [R.from_mont_words(R.from_bytes(t.root)) for t in round_trees]

    # ---- prover
    ch = F.DuplexChallenger(external)
    for c in commits:
        ch.observe(c)
    zeta = ch.sample_ext()
    verifier_start = ch.clone()
    alpha = ch.sample_ext()
    fri = FriOpening(log_blowup, external)
    assert fri.begin(F.to_bytes(alpha))
    opened = []
    for mats, ds in zip(ldes, devs):
        ys = fri.add_round_ptr([(d.ptr, m.shape[0], cols) for d, m in zip(ds, mats)],
                               [[F.to_bytes(zeta)]] * len(mats))
        assert ys is not None
        opened.append([[F.from_bytes(y) for y in per_matrix] for per_matrix in ys])
    log_max = fri.input_log_size(0)

    def on_commit(root):
        ch.observe(R.from_mont_words(R.from_bytes(root)))
        return F.to_bytes(ch.sample_ext())

    roots = [R.from_mont_words(R.from_bytes(r)) for r in fri.commit_phase(on_commit)]
    final_eval = F.from_bytes(fri.final_eval)[0]
    ch.observe(final_eval)
    witness = ch.grind(pow_bits)
    queries = []
    for _ in range(num_queries):
        index = ch.sample_bits(log_max)
        input_proof = []
        for t, mats in zip(round_trees, ldes):
            log_round = max(m.shape[0] for m in mats).bit_length() - 1
            rows, sibs = t.open(index >> (log_max - log_round))
            input_proof.append(([R.from_mont_words(R.from_bytes(r)) for r in rows],
                                [R.from_mont_words(R.from_bytes(s)) for s in sibs]))
        answers = [(F.from_bytes(v)[0], [R.from_mont_words(R.from_bytes(s)) for s in sibs])
                   for v, sibs in fri.answer_query(index)]
        queries.append((input_proof, answers))

    # ---- verifier (fri::Verify and VerifyOpeningProof's callback)
    v = verifier_start
    v_alpha = v.sample_ext()
    assert (v_alpha == alpha).all()
    assert len(roots) == log_max - log_blowup
    v_betas = []
    for root in roots:
        v.observe(root)
        v_betas.append(v.sample_ext())
    v.observe(final_eval)
    assert v.check_witness(pow_bits, witness)
    for input_proof, answers in queries:
        index = v.sample_bits(log_max)
        rounds = []
        for (rows, sibs), mats, commit, ys in zip(input_proof, ldes, commits, opened):
            log_round = max(m.shape[0] for m in mats).bit_length() - 1
            dims = [(m.shape[0], cols) for m in mats]
            assert R.verify(commit, dims, index >> (log_max - log_round), rows, sibs, external)
            rounds.append([(m.shape[0].bit_length() - 1, [zeta], y, row) for m, y, row in zip(mats, ys, rows)])
        reduced = F.verifier_reduced_openings(index, log_max, alpha, rounds)
        folded = F.verify_query(index, log_max, v_betas, roots, answers, reduced, external)
        assert folded is not None and (folded == final_eval).all()
    fri.close()
