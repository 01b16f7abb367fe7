"""The KZG opening reference (tests/kzg_open_ref.py) against itself and the
reference implementation's fixture: its polynomial arithmetic is consistent,
and what its provers produce its verifiers accept -- under both schemes and
both readings of the fixture (36 polynomials by index; 18 with equal
coefficient vectors merged, the only reading with multi-point groups) -- and
reject once a claimed value is changed.  No GPU, no library."""
import os
import random

import pytest

import kzg_open_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn254_kzg_polynomial_openings.json")
CURVE = "bn254_g1"
TAU = 2  # kzg_family_test.h: UnsafeSetup(N = 16, tau = 2)


@pytest.fixture(scope="module")
def grp():
    return R.Group(CURVE)


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture(GOLDEN)


def readings(fixture):
    polys, openings, _ = fixture
    return {"by_index": (polys, openings), "merged": R.merge_equal(polys, openings)}


def test_fixture_is_what_the_issue_says(fixture, grp):
    polys, openings, commitments = fixture
    assert len(polys) == 36 and all(len(p) == 16 for p in polys)
    assert len({x for _, x, _ in openings}) == 3
    for (i, x, v), c in zip(openings, commitments):
        assert R.evaluate(polys[i], x, grp.r) == v
    for i in (0, 17, 35):  # the commitments are [P(2)]G
        assert grp.C.from_bytes(grp.commit(TAU)(polys[i])) == commitments[i]
    by_index = R.group_by_poly_and_points(openings)
    assert [(len(g[0]), len(g[1])) for g in by_index] == [(1, 20), (1, 10), (1, 6)]
    merged, mo = R.merge_equal(polys, openings)
    assert len(merged) == 18
    assert sorted((len(g[0]), len(g[1])) for g in R.group_by_poly_and_points(mo)) == [(1, 9), (2, 3), (3, 6)]
    assert [len(g[1]) for g in R.group_by_single_point(mo)] == [20, 10, 6]


def test_polynomial_arithmetic():
    r = R.Group(CURVE).r
    rng = random.Random(11)
    for n in (0, 1, 2, 5, 17):
        p = [rng.randrange(r) for _ in range(n)]
        for roots in ([3], [0], [r - 1, 5], [7, 7, 9], [1, 2, 3, 4, 5]):
            q, rems = R.divide_by_roots(p, roots, r)
            assert len(q) == max(0, n - len(roots)) and len(rems) == len(roots)
            assert q == R.long_division(p, R.from_roots(roots, r), r)
            assert rems[0] == R.evaluate(p, roots[0], r)
            # exact division: quotient x vanishing divides back with zero remainders
            z = R.from_roots(roots, r)
            prod = [0] * (len(p) + len(z) - 1) if p else []
            for i, a in enumerate(p):
                for j, b in enumerate(z):
                    prod[i + j] = (prod[i + j] + a * b) % r
            q2, rems2 = R.divide_by_roots(prod, roots, r)
            assert q2 == p and not any(rems2)
    xs, ys = [5, 9, 2], [rng.randrange(r) for _ in range(3)]
    interp = R.lagrange_interpolate(xs, ys, r)
    assert [R.evaluate(interp, x, r) for x in xs] == ys
    assert R.linear_combination([[1, 2, 3], [], [4]], [2, 9, 3], 5, r) == [(2 + 12 - 5) % r, 4, 6]


@pytest.mark.parametrize("reading", ["by_index", "merged"])
@pytest.mark.parametrize("scheme", [R.GWC, R.SHPLONK])
def test_prove_then_verify(fixture, grp, scheme, reading):
    polys, openings = readings(fixture)[reading]
    prove, verify = (R.gwc_prove, R.gwc_verify) if scheme == R.GWC else (R.shplonk_prove, R.shplonk_verify)
    commit = grp.commit(TAU)
    t = R.Transcript(CURVE)
    quotients = prove(polys, openings, t, commit, grp.r)
    proof = [commit(w) for w in quotients]
    assert [c[0] for c in t.calls] == (["squeeze"] + ["write"] * len(proof) if scheme == R.GWC else
                                       ["squeeze", "squeeze", "write", "squeeze", "write"])
    commitments = [commit(p) for p in polys]
    assert verify(grp, TAU, commitments, openings, proof, R.Transcript(CURVE))
    # one claimed value changed: the prover's remainder is dropped, the verifier refuses
    i, x, v = openings[5]
    bad = openings[:5] + [(i, x, (v + 1) % grp.r)] + openings[6:]
    bad_proof = [commit(w) for w in prove(polys, bad, R.Transcript(CURVE), commit, grp.r)]
    assert not verify(grp, TAU, commitments, bad, bad_proof, R.Transcript(CURVE))
    # and the honest proof does not fit the changed claim either
    assert not verify(grp, TAU, commitments, bad, proof, R.Transcript(CURVE))


def test_shplonk_algebra_identity(fixture, grp):
    """(tau - u) Q(tau) Z_{T\\0}(u) = L(tau), the identity behind the final check, on the merged reading."""
    polys, openings = readings(fixture)["merged"]
    r = grp.r
    t = R.Transcript(CURVE)
    h, q = R.shplonk_prove(polys, openings, t, lambda p: grp.zero, r)
    y, v, u = [c[1] for c in t.calls if c[0] == "squeeze"]
    groups, sup = R.group_by_poly_and_points(openings), R.super_points(openings)
    l_tau = 0
    for g, (pts, idx, vals) in enumerate(groups):
        z_diff = R.vanishing_at([x for x in sup if x not in pts], u, r)
        inner = sum(pow(y, j, r) * (R.evaluate(polys[i], TAU, r) - R.evaluate(R.lagrange_interpolate(pts, val, r), u, r))
                    for j, (i, val) in enumerate(zip(idx, vals)))
        l_tau += pow(v, g, r) * z_diff * inner
    l_tau = (l_tau - R.vanishing_at(sup, u, r) * R.evaluate(h, TAU, r)) % r
    z0 = R.vanishing_at([x for x in sup if x not in groups[0][0]], u, r)
    assert (TAU - u) * R.evaluate(q, TAU, r) * z0 % r == l_tau


def test_failures(fixture, grp):
    polys, openings = readings(fixture)["merged"]
    commit = grp.commit(TAU)
    assert R.gwc_prove(polys, openings, R.Transcript(CURVE, fail_write=1), commit, grp.r) is None
    assert R.shplonk_prove(polys, openings, R.Transcript(CURVE, fail_write=0), commit, grp.r) is None
    groups = R.group_by_poly_and_points(openings)
    outside = next(x for x in R.super_points(openings) if x not in groups[0][0])
    assert R.shplonk_prove(polys, openings, R.Transcript(CURVE, force={2: outside}), commit, grp.r) is None
    i, x, v = openings[0]
    assert R.group_by_poly_and_points(openings + [(i, x, v + 1)]) is None
    assert R.group_by_poly_and_points(openings + [(i, x, v)]) == groups
