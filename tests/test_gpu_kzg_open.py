"""KZG openings on the GPU: the three polynomial kernel families at their
edges (tachyon_mi355x_kzg_poly_divide_by_roots / _poly_linear_combination /
_evaluate_batch) and the GWC / SHPlonk CreateOpeningProof in one call, all
against tests/kzg_open_ref.py, bytes for bytes.

Tiling constants of the kernels (csrc/kzg/poly_ops.h): 8 coefficients per
thread (chunk), 64 threads per wave, 256 threads = 2048 coefficients per
workgroup (tile); the division's carry pass is one workgroup that walks the
per-tile carries 2048 at a time (carry chunk), so tile x carry chunk + 1 =
4,194,305 coefficients is the first length at which it takes a second step
(and the evaluation a third level).

The kernels are linear in the coefficients, so the reference runs directly on
the Montgomery integers of the inputs (with canonical roots / factors) and its
results are the Montgomery integers of the outputs: no conversion per element.
"""
import os
import random

import numpy as np
import pytest

import kzg_open_ref as R
from oracle import oracle as O
from oracle import pyref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn254_kzg_polynomial_openings.json")
FIELDS = {"bn254_g1": "bn254_fr", "bls12_381_g1": "bls12_381_fr"}
LENGTHS = list(range(131)) + [(1 << k) + d for k in range(7, 18) for d in (-1, 0, 1)]
TILE, CARRY_CHUNK = 2048, 2048


def ints(b):
    """32-byte little-endian words -> integers (Montgomery integers of Montgomery bytes)."""
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def raw(xs):
    return b"".join(x.to_bytes(32, "little") for x in xs)


def rand_poly(field, seed, n):
    """n random elements as Montgomery bytes (the oracle's generator)."""
    return O.gen_scalars(field, seed, n).tobytes() if n else b""


def special_roots(F, seed):
    rng = random.Random(seed)
    return [0, 1, F.p - 1, F.root_of_unity(1 << 16), rng.randrange(F.p)]


# --- division ---------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254_g1", "bls12_381_g1"])
def test_divide_every_length(curve):
    """Lengths 0..130 and 2^k - 1, 2^k, 2^k + 1 for k = 7..17 (chunk, wave, tile
    boundaries), one root each from {0, 1, r - 1, a domain root, random}:
    inexact divisions, quotient and remainder equal the reference's."""
    from tachyon_amd.kzg import poly_divide_by_roots
    F = pyref.Field(FIELDS[curve])
    roots = special_roots(F, 1)
    pool = rand_poly(F.name, 41, max(LENGTHS))
    pool_ints = ints(pool)
    for k, n in enumerate(LENGTHS):
        z = roots[k % len(roots)]
        q, rems = poly_divide_by_roots(curve, pool[:32 * n], [F.to_bytes(z)])
        want_q, want_r = R.divide_by_roots(pool_ints[:n], [z], F.p)
        assert q == raw(want_q), (n, z)
        assert rems == [raw(want_r)], (n, z)


@pytest.mark.parametrize("curve", ["bn254_g1", "bls12_381_g1"])
def test_divide_root_lists(curve):
    """Root lists of 1, 2, 3 and 5 roots (a repeated root among them, and more
    roots than coefficients): the roots are applied one after another on the
    device; every step's remainder equals the reference's."""
    from tachyon_amd.kzg import poly_divide_by_roots
    F = pyref.Field(FIELDS[curve])
    z0, z1, zm, zw, zr = special_roots(F, 2)
    lists = [[zr], [zw, zr], [zr, zr, z1], [z0, zr, zm, zr, zw]]
    for n in (0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 130, 511, 513, 2047, 2048, 2049, 2053, 4097, 3 * TILE + 2):
        a = rand_poly(F.name, 50 + n, n)
        for roots in lists:
            q, rems = poly_divide_by_roots(curve, a, [F.to_bytes(z) for z in roots])
            want_q, want_r = R.divide_by_roots(ints(a), roots, F.p)
            assert len(q) == 32 * max(0, n - len(roots))
            assert q == raw(want_q) and rems == [raw([x]) for x in want_r], (n, roots)


@pytest.mark.parametrize("curve", ["bn254_g1", "bls12_381_g1"])
def test_divide_exact_and_zero(curve):
    """Numerator = quotient x vanishing polynomial: the quotient comes back and
    every remainder is zero; the zero polynomial divides to zero."""
    from tachyon_amd.kzg import poly_divide_by_roots
    F = pyref.Field(FIELDS[curve])
    z0, z1, zm, zw, zr = special_roots(F, 3)
    for n in (1, 2, 17, 129, 2046, 2048, 4099):
        quot = ints(rand_poly(F.name, 70 + n, n))
        for roots in ([zw], [zr, z0], [zm, zr, zr], [z1, zw, zr, zm, zw]):
            van = R.from_roots(roots, F.p)
            num = [0] * (n + len(roots))
            for j, c in enumerate(van):  # quotient x vanishing, a shifted sum per vanishing coefficient
                for i, a in enumerate(quot):
                    num[i + j] = (num[i + j] + a * c) % F.p
            q, rems = poly_divide_by_roots(curve, raw(num), [F.to_bytes(z) for z in roots])
            assert q == raw(quot) and rems == [bytes(32)] * len(roots), (n, roots)
    for n in (1, 5, 2049):
        q, rems = poly_divide_by_roots(curve, bytes(32 * n), [F.to_bytes(zr), F.to_bytes(zw)])
        assert q == bytes(32 * max(0, n - 2)) and rems == [bytes(32)] * 2


def sparse_suffix_bytes(n, vals, z, r):
    """The bytes of S_j = a_j + z S_(j+1), j < n, for the sparse a = {position:
    value} and z of order 4: between two nonzero coefficients S_j = z^(top - j)
    S_top runs through a 4-cycle, laid down as a repeated block."""
    out = bytearray(32 * n)
    cur, top = 0, n  # S_top, everything from top upwards is filled
    for p in sorted(vals, reverse=True) + [-1]:
        gap = top - 1 - p
        if gap and cur:
            cyc = [cur * pow(z, t, r) % r for t in range(1, 5)]  # t = top - j
            out[32 * (p + 1):32 * top] = (raw([cyc[3], cyc[2], cyc[1], cyc[0]]) * (gap // 4 + 1))[-32 * gap:]
        if p >= 0:
            cur = (vals[p] + pow(z, gap + 1, r) * cur) % r
            out[32 * p:32 * p + 32] = cur.to_bytes(32, "little")
            top = p
    return out


def test_divide_and_evaluate_past_the_carry_chunk():
    """tile x carry chunk + 1 coefficients: the carry pass takes a second step
    and the evaluation a third level.  The polynomial is sparse and the root a
    4th root of unity, so the reference quotient is piecewise a 4-cycle and is
    built without 4M big-integer products."""
    import torch
    from tachyon_amd.kzg import KZG, poly_divide_by_roots
    F = pyref.Field("bn254_fr")
    r, n = F.p, TILE * CARRY_CHUNK + 1
    z = F.root_of_unity(4)
    rng = random.Random(9)
    pos = sorted({0, 1, 7, 8, TILE - 1, TILE, TILE + 1, TILE * CARRY_CHUNK - 1, TILE * CARRY_CHUNK,
                  n - 2 * TILE - 3} | {rng.randrange(n) for _ in range(30)}, reverse=True)
    vals = {p: rng.randrange(1, r) for p in pos}  # Montgomery integers
    a = bytearray(32 * n)
    for p, v in vals.items():
        a[32 * p:32 * p + 32] = v.to_bytes(32, "little")
    s_bytes = sparse_suffix_bytes(n, vals, z, r)
    want_q, want_rem = bytes(s_bytes[32:]), bytes(s_bytes[:32])
    d = torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).cuda()
    q, rems = poly_divide_by_roots("bn254_g1", d, [F.to_bytes(z)])
    assert rems == [want_rem]
    assert q == want_q
    kzg = KZG("bn254_g1")
    assert kzg.evaluate([d], [(0, F.to_bytes(z))]) == [want_rem]
    kzg.close()


# --- linear combination -------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254_g1", "bls12_381_g1"])
@pytest.mark.parametrize("count", [1, 2, 17, 64])
def test_linear_combination(curve, count):
    """1, 2, 17 and 64 inputs of ragged lengths (0 and 1 among them),
    coefficients 0 and 1 among random ones, the constant term, host and device
    inputs mixed, and a device output."""
    import torch
    from tachyon_amd.kzg import poly_linear_combination
    F = pyref.Field(FIELDS[curve])
    rng = random.Random(count)
    lens = [rng.choice([0, 1, 2, 255, 256, 257, 1000, 2049, 4500]) for _ in range(count)]
    lens[0] = 4500 if count > 1 else 257
    if count > 2:
        lens[1], lens[2] = 0, 1
    polys = [rand_poly(F.name, 100 + i, n) for i, n in enumerate(lens)]
    coeffs = [rng.randrange(F.p) for _ in range(count)]
    if count > 2:
        coeffs[3], coeffs[4] = 0, 1
    d = rng.randrange(F.p)
    want = raw(R.linear_combination([ints(p) for p in polys], coeffs, int.from_bytes(F.to_bytes(d), "little"), F.p))
    mixed = [torch.from_numpy(np.frombuffer(p, np.uint8).copy()).cuda() if i % 2 == 0 and p else p
             for i, p in enumerate(polys)]
    cb = [F.to_bytes(c) for c in coeffs]
    assert poly_linear_combination(curve, mixed, cb, F.to_bytes(d)) == want
    assert poly_linear_combination(curve, polys, cb, F.to_bytes(d)) == want
    out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    poly_linear_combination(curve, mixed, cb, F.to_bytes(d), out=out)
    assert out.cpu().numpy().tobytes() == want
    # no constant
    assert poly_linear_combination(curve, mixed, cb) == raw(R.linear_combination([ints(p) for p in polys], coeffs, 0, F.p))


def cuda_off_by_4(b):
    """A CUDA tensor holding b that starts 4 bytes past a 16-byte boundary."""
    import torch
    view = torch.empty(len(b) + 16, dtype=torch.uint8, device="cuda")[4:4 + len(b)]
    view.copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("n", [3, 257])
def test_staged_inputs_and_output(n):
    """What the kernels cannot use in place is staged: one host array passed
    twice, a device polynomial and a device output that are not 16-byte
    aligned; 257 is one past a workgroup's threads."""
    from tachyon_amd.kzg import poly_divide_by_roots, poly_linear_combination
    F = pyref.Field("bn254_fr")
    rng = random.Random(n)
    a, b = rand_poly(F.name, 120, n), rand_poly(F.name, 121, n)
    twice, unaligned = np.frombuffer(a, np.uint8), cuda_off_by_4(b)
    coeffs = [rng.randrange(F.p) for _ in range(3)]
    d = rng.randrange(F.p)
    want = raw(R.linear_combination([ints(a), ints(a), ints(b)], coeffs, int.from_bytes(F.to_bytes(d), "little"), F.p))
    out = cuda_off_by_4(bytes(32 * n))
    got = poly_linear_combination("bn254_g1", [twice, twice, unaligned], [F.to_bytes(c) for c in coeffs], F.to_bytes(d),
                                  out=out)
    assert got is out and out.cpu().numpy().tobytes() == want
    z = rng.randrange(F.p)
    q, rems = poly_divide_by_roots("bn254_g1", unaligned, [F.to_bytes(z)])
    want_q, want_r = R.divide_by_roots(ints(b), [z], F.p)
    assert q == raw(want_q) and rems == [raw(want_r)]


# --- evaluation -----------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254_g1", "bls12_381_g1"])
def test_evaluate_batch(curve):
    """One batch over polynomials of every length of the list, each at one of
    {0, 1, r - 1, random}; the long ones at all four; the empty polynomial is 0."""
    from tachyon_amd.kzg import KZG
    F = pyref.Field(FIELDS[curve])
    rng = random.Random(4)
    points = [0, 1, F.p - 1, rng.randrange(F.p)]
    pool = rand_poly(F.name, 43, max(LENGTHS))
    pool_ints = ints(pool)
    polys = [pool[32 * (k % 5):][:32 * n] for k, n in enumerate(LENGTHS)]  # different windows of the pool
    pairs = [(k, points[k % 4]) for k in range(len(LENGTHS))]
    pairs += [(k, z) for k in range(len(LENGTHS) - 4, len(LENGTHS)) for z in points]
    pairs += [(0, points[3]), (1, points[3])]
    kzg = KZG(curve)
    got = kzg.evaluate(polys, [(k, F.to_bytes(z)) for k, z in pairs])
    want = [R.evaluate(pool_ints[k % 5:][:LENGTHS[k]], z, F.p).to_bytes(32, "little") for k, z in pairs]
    assert got == want
    assert got[0] == bytes(32) and kzg.evaluate([b""], [(0, F.to_bytes(5))]) == [bytes(32)]
    assert kzg.evaluate(polys, []) == []
    assert kzg.evaluate(polys[:3], [(3, F.to_bytes(1))]) is None  # index out of range
    kzg.close()


# --- proofs ---------------------------------------------------------------------------
def to_bytes_poly(F, p):
    return b"".join(F.to_bytes(c) for c in p)


def lib_openings(F, openings):
    return [(i, F.to_bytes(x), F.to_bytes(v)) for i, x, v in openings]


def check_proof(kzg, curve, tau, polys, openings, scheme, device=False):
    """The library's proof equals [W(tau)]G of the reference's quotients, the
    reference verifier accepts it, and the callbacks came in the reference's order."""
    import torch
    grp = R.Group(curve)
    F = grp.C.Fr
    commit = grp.commit(tau)
    prove, verify = (R.gwc_prove, R.gwc_verify) if scheme == R.GWC else (R.shplonk_prove, R.shplonk_verify)
    ref_t = R.Transcript(curve)
    want = [commit(w) for w in prove(polys, openings, ref_t, commit, grp.r)]
    pb = [to_bytes_poly(F, p) for p in polys]
    if device:
        pb = [torch.from_numpy(np.frombuffer(p, np.uint8).copy()).cuda() if p else p for p in pb]
    t = R.Transcript(curve)
    got = kzg.create_opening_proof(pb, lib_openings(F, openings), t, scheme=scheme)
    assert got == want
    assert t.calls == ref_t.calls  # the same challenges squeezed and points written, in the same order
    kinds = [c[0] for c in t.calls]
    assert kinds == (["squeeze"] + ["write"] * len(want) if scheme == R.GWC else
                     ["squeeze", "squeeze", "write", "squeeze", "write"])
    assert verify(grp, tau, [commit(p) for p in polys], openings, got, R.Transcript(curve))
    return got


@pytest.fixture(scope="module")
def kzg16():
    from tachyon_amd.kzg import KZG
    kzg = KZG("bn254_g1")
    kzg.unsafe_setup(16, pyref.Field("bn254_fr").to_bytes(2))
    yield kzg
    kzg.close()


@pytest.mark.parametrize("reading", ["by_index", "merged"])
@pytest.mark.parametrize("scheme", [R.GWC, R.SHPLONK])
def test_fixture_proofs(kzg16, scheme, reading):
    polys, openings, commitments = R.load_fixture(GOLDEN)
    # the fixture's own commitments are what this SRS commits to
    got = kzg16.commit_batch([to_bytes_poly(pyref.Field("bn254_fr"), p) for p in polys[:4]])
    C = pyref.Curve("bn254_g1")
    assert [C.from_bytes(c) for c in got] == commitments[:4]
    if reading == "merged":
        polys, openings = R.merge_equal(polys, openings)
    check_proof(kzg16, "bn254_g1", 2, polys, openings, scheme)


@pytest.fixture(scope="module")
def kzg8k():
    from tachyon_amd.kzg import KZG
    kzg = KZG("bn254_g1")
    kzg.unsafe_setup(1 << 13, pyref.Field("bn254_fr").to_bytes(0xABCDEF1234567))
    yield kzg
    kzg.close()


def ragged_case(r, n):
    rng = random.Random(13)
    polys = [[rng.randrange(r) for _ in range(l)] for l in (n, n - 1, 4097, 1, 0, n)]
    xs = [rng.randrange(r) for _ in range(3)]
    pairs = [(0, xs[0]), (1, xs[1]), (2, xs[0]), (3, xs[2]), (4, xs[1]), (5, xs[0]), (0, xs[2]), (2, xs[0])]
    return polys, [(i, x, R.evaluate(polys[i], x, r)) for i, x in pairs]


@pytest.mark.parametrize("scheme", [R.GWC, R.SHPLONK])
def test_proof_past_one_workgroup(kzg8k, scheme):
    """N = 2^13, six polynomials of lengths (N, N - 1, 4097, 1, 0, N), three
    points, polynomial 0 opened at two of them, one opening repeated; device-
    resident polynomials."""
    r = pyref.Field("bn254_fr").p
    polys, openings = ragged_case(r, 1 << 13)
    check_proof(kzg8k, "bn254_g1", 0xABCDEF1234567, polys, openings, scheme, device=True)


@pytest.mark.parametrize("scheme", [R.GWC, R.SHPLONK])
def test_proof_bls12_381(scheme):
    from tachyon_amd.kzg import KZG
    F = pyref.Field("bls12_381_fr")
    n, tau = 1 << 6, 0x1357924680
    rng = random.Random(17)
    polys = [[rng.randrange(F.p) for _ in range(l)] for l in (n, 33, n - 1, 2)]
    xs = [rng.randrange(F.p) for _ in range(3)]
    pairs = [(0, xs[0]), (1, xs[0]), (0, xs[1]), (1, xs[1]), (2, xs[2]), (3, xs[0])]
    openings = [(i, x, R.evaluate(polys[i], x, F.p)) for i, x in pairs]
    kzg = KZG("bls12_381_g1")
    kzg.unsafe_setup(n, F.to_bytes(tau))
    check_proof(kzg, "bls12_381_g1", tau, polys, openings, scheme)
    kzg.close()


def test_proof_failures(kzg16):
    """Where the reference returns false or CHECKs, the call returns None: a
    failed write, u at a point outside the first group (Z_{T\\0}(u) = 0), more
    coefficients than N, an index out of range, conflicting SHPlonk claims."""
    F = pyref.Field("bn254_fr")
    polys, openings, _ = R.load_fixture(GOLDEN)
    polys, openings = R.merge_equal(polys, openings)
    pb = [to_bytes_poly(F, p) for p in polys]
    lo = lib_openings(F, openings)
    for scheme, nwrites in ((R.GWC, 3), (R.SHPLONK, 2)):
        for k in range(nwrites):
            t = R.Transcript("bn254_g1", fail_write=k)
            assert kzg16.create_opening_proof(pb, lo, t, scheme=scheme) is None
            assert t.writes == k + 1  # nothing is written after the failed write
    groups = R.group_by_poly_and_points(openings)
    outside = next(x for x in R.super_points(openings) if x not in groups[0][0])
    t = R.Transcript("bn254_g1", force={2: outside})
    assert kzg16.create_opening_proof(pb, lo, t, scheme="shplonk") is None
    assert [c[0] for c in t.calls] == ["squeeze", "squeeze", "write", "squeeze"]
    inside = groups[0][0][0]  # u at a point of the first group is no failure
    t = R.Transcript("bn254_g1", force={2: inside})
    assert kzg16.create_opening_proof(pb, lo, t, scheme="shplonk") is not None
    for scheme in (R.GWC, R.SHPLONK):
        for bad_polys, bad_open in ((pb[:-1] + [pb[-1] + F.to_bytes(1)], lo),  # 17 coefficients, N = 16
                                    (pb, lo + [(len(pb), F.to_bytes(1), F.to_bytes(1))])):
            t = R.Transcript("bn254_g1")
            assert kzg16.create_opening_proof(bad_polys, bad_open, t, scheme=scheme) is None
            assert t.calls == []  # refused before any callback
    # no opening at all: GWC squeezes v and writes nothing, SHPlonk has no first group to normalise by
    t = R.Transcript("bn254_g1")
    assert kzg16.create_opening_proof(pb, [], t, scheme="gwc") == [] and [c[0] for c in t.calls] == ["squeeze"]
    t = R.Transcript("bn254_g1")
    assert kzg16.create_opening_proof(pb, [], t, scheme="shplonk") is None and t.calls == []
    i, x, v = lo[0]
    t = R.Transcript("bn254_g1")
    assert kzg16.create_opening_proof(pb, lo + [(i, x, F.to_bytes(12345))], t, scheme="shplonk") is None and t.calls == []
    assert kzg16.create_opening_proof(pb, lo + [(i, x, F.to_bytes(12345))], R.Transcript("bn254_g1"), scheme="gwc")


@pytest.mark.parametrize("scheme", [R.GWC, R.SHPLONK])
def test_evaluate_then_prove(kzg8k, scheme):
    """The prover's own evaluations fed straight back as the claimed values give
    the proof the reference's values give."""
    F = pyref.Field("bn254_fr")
    polys, openings = ragged_case(F.p, 1 << 13)
    pb = [to_bytes_poly(F, p) for p in polys]
    values = kzg8k.evaluate(pb, [(i, F.to_bytes(x)) for i, x, _ in openings])
    assert values == [F.to_bytes(v) for _, _, v in openings]
    mine = kzg8k.create_opening_proof(pb, [(i, F.to_bytes(x), v) for (i, x, _), v in zip(openings, values)],
                                      R.Transcript("bn254_g1"), scheme=scheme)
    theirs = kzg8k.create_opening_proof(pb, lib_openings(F, openings), R.Transcript("bn254_g1"), scheme=scheme)
    assert mine is not None and mine == theirs
    ms = kzg8k.last_open_timings()
    assert set(ms) == {"evaluate", "combine", "divide", "commit"} and ms["commit"] > 0
