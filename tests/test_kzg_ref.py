"""CPU-side checks of tests/kzg_ref.py (no GPU): the Lagrange coefficients it
hands the KZG GPU tests satisfy the identities of a Lagrange basis -- partition
of unity, sum L_i w^i = tau, L_i(w^j) = [i == j], interpolation of a random
polynomial -- on both scalar fields, at every size and trapdoor the GPU tests
use; and its two point routines (the oracle's multiplication, pyref's) agree."""
import random

import pytest

import kzg_ref as K
from oracle import pyref

FIELDS = ["bn254_fr", "bls12_381_fr"]
SIZES = [1, 2, 8, 512]
TAUS = ["0", "1", "2", "r-1", "w^(n-1)", "0x123456789abcdef0"]


def trapdoor(Fr, n, name):
    if name == "r-1":
        return Fr.p - 1
    if name == "w^(n-1)":
        return pow(Fr.root_of_unity(n), n - 1, Fr.p)
    return int(name, 0)


@pytest.mark.parametrize("tau_name", TAUS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("field", FIELDS)
def test_lagrange_identities(field, n, tau_name):
    Fr = pyref.Field(field)
    r = Fr.p
    w = Fr.root_of_unity(n)
    tau = trapdoor(Fr, n, tau_name)
    powers, lag = K.srs_scalars(field, n, tau)
    assert len(powers) == len(lag) == n
    assert powers == [pow(tau, i, r) for i in range(n)]
    assert all(0 <= v < r for v in lag)
    assert sum(lag) % r == 1
    if n >= 2:
        assert sum(l * pow(w, i, r) for i, l in enumerate(lag)) % r == tau
    # sum_i p(w^i) L_i(tau) = p(tau) for deg p < n: with the two sums above
    # (p = 1 and p = x) this pins every coefficient, not only their total
    rng = random.Random(n)
    p = [rng.randrange(r) for _ in range(n)]
    assert sum(horner(p, pow(w, i, r), r) * l for i, l in enumerate(lag)) % r == horner(p, tau, r)


def horner(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % r
    return acc


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("field", FIELDS)
def test_lagrange_at_domain_points(field, n):
    """L_i(w^j) = [i == j]: every j at n <= 8, the ends, the middle and a few
    more at 512."""
    Fr = pyref.Field(field)
    w = Fr.root_of_unity(n)
    js = range(n) if n <= 8 else [0, 1, 255, 256, 257, n - 2, n - 1]
    for j in js:
        _, lag = K.srs_scalars(field, n, pow(w, j, Fr.p))
        assert lag == [1 if i == j else 0 for i in range(n)], j


@pytest.mark.parametrize("n", [2, 512])
@pytest.mark.parametrize("field", FIELDS)
def test_named_trapdoors_in_the_domain(field, n):
    """1, r - 1 and w^(n-1) are w^0, w^(n/2) and w^(n-1)."""
    Fr = pyref.Field(field)
    for name, j in (("1", 0), ("r-1", n // 2), ("w^(n-1)", n - 1)):
        _, lag = K.srs_scalars(field, n, trapdoor(Fr, n, name))
        assert lag.index(1) == j and sum(lag) == 1, name


@pytest.mark.parametrize("curve", sorted(K.SCALAR_FIELD))
def test_point_routines_agree(curve):
    """The oracle's [k]G and pyref's, at the scalars where a multiplication goes
    wrong first: 0, 1, 2, r - 1, a single high bit, a full-width value."""
    r = pyref.Curve(curve).Fr.p
    scalars = [0, 1, 2, r - 1, pow(2, 511, r), 1 << 250, (r - 1) // 2, 0x123456789abcdef0, pow(3, 200, r)]
    pts = K.srs_points(curve, scalars)
    pb = pyref.Curve(curve).point_bytes
    assert len(pts) == pb * len(scalars)
    spot = K.spot_points(curve, scalars, range(len(scalars)))
    for i in range(len(scalars)):
        assert pts[i * pb:(i + 1) * pb] == spot[i], i
    C = pyref.Curve(curve)
    assert spot[0] == bytes(pb) and spot[1] == C.to_bytes(C.G) and spot[3] == C.to_bytes(C.neg(C.G))
