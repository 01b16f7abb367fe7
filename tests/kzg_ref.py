"""The reference the KZG GPU tests compare against: the SRS scalars tau^i and
L_i(tau) as plain Python integers, and the SRS points [k]G through the oracle's
scalar multiplication (all of them) or the pure-Python curve of oracle/pyref.py
(a few spot indices).  It does not import the library.

Conventions (the reference's UnsafeSetup, kzg.h:173-207): the Lagrange basis is
over the size-n radix-2 domain <w>, w = Field.root_of_unity(n),

    L_i(tau) = (tau^n - 1) / n * w^i / (tau - w^i)

and when tau lies in the domain (tau^n = 1) it is the indicator of the j with
w^j = tau (EvaluateAllLagrangeCoefficients, univariate_evaluation_domain.h:
309-323).  Points are affine Montgomery bytes, the identity all zero.
"""
import functools

from oracle import oracle as O
from oracle import pyref

SCALAR_FIELD = {"bn254_g1": "bn254_fr", "bls12_381_g1": "bls12_381_fr"}


def srs_scalars(field, n, tau):
    """([tau^i mod r], [L_i(tau)]) for i < n, canonical integers."""
    Fr = pyref.Field(field)
    r = Fr.p
    tau %= r
    w = Fr.root_of_unity(n)
    powers, domain = [], []
    t = wi = 1
    for _ in range(n):
        powers.append(t)
        domain.append(wi)
        t = t * tau % r
        wi = wi * w % r
    z = (pow(tau, n, r) - 1) % r
    if z == 0:
        return powers, [1 if wi == tau else 0 for wi in domain]
    z_over_n = z * pow(n, -1, r) % r
    return powers, [z_over_n * wi * pow((tau - wi) % r, -1, r) % r for wi in domain]


@functools.lru_cache(maxsize=None)
def _mul_g(curve, k):
    C = pyref.Curve(curve)
    return O.ec_op(curve, "mul", C.to_bytes(C.G), k.to_bytes(32, "little"))  # plain-integer scalar


def srs_points(curve, scalars):
    """[k]G for every k, concatenated affine bytes (the oracle's multiplication)."""
    return b"".join(_mul_g(curve, int(k)) for k in scalars)


def spot_points(curve, scalars, indices):
    """{i: [scalars[i]]G} by pyref's textbook affine double-and-add."""
    C = pyref.Curve(curve)
    return {i: C.to_bytes(C.mul(C.G, int(scalars[i]))) for i in indices}
