"""Synthetic circom proving keys for the Groth16 parity tests and the bench
(test infrastructure; the reference's stand-in is ToxicWaste::RandomWithoutX,
vendors/circom/circomlib/circuit/circuit_test.h:34-49).

synth_zkey: the points are seeded k*G doubling chains (oracle.gen_bases: valid
curve points, no trapdoor), the coefficients random, so the proofs are not
verifiable -- they pin the GPU prover to the CPU oracle bit for bit.  The
reference's multiplier_3.zkey and adder.zkey cover verifiability at their
sizes (tests/test_groth16_oracle.py).

trapdoor_zkey: a real BN254 setup from a seeded trapdoor and an R1CS, so its
proofs pass the pairing check (oracle/bn254_pairing.py) at any size;
random_r1cs makes a satisfied R1CS for it.
"""
import random

from oracle import oracle as O
from oracle import pyref
from oracle.circom_format import CURVE_FIELDS, write_zkey

CURVE_NAMES = {"bn254": ("bn254_g1", "bn254_g2", "bn254_fr"),
               "bls12_381": ("bls12_381_g1", "bls12_381_g2", "bls12_381_fr")}


def synth_zkey(curve="bn254", log_n=6, num_vars=None, num_public=2, nnz_per_row=3, seed=1, empty_rows=0.1,
               coefficients=None, full=None):
    """Returns (zkey bytes, full assignment as canonical ints).
    coefficients: the (matrix, constraint, signal, word bytes) list to write
    instead of the random rows (the edge tests' hand-made row shapes);
    full: {signal: value} overrides of the random assignment."""
    g1n, g2n, frn = CURVE_NAMES[curve]
    q, r, n8q, n8r = CURVE_FIELDS[curve]
    rng = random.Random(seed)
    n = 1 << log_n
    m = num_vars if num_vars is not None else max(num_public + 1, n - n // 4)
    pb1 = 2 * n8q

    def pts(c, k, s):
        if k == 0:
            return b""
        return O.gen_bases(c, s, k, max(1, k // 3)).tobytes()

    g1 = pts(g1n, 5 + num_public + 1 + 3 * m + n, seed * 7 + 1)
    g2 = pts(g2n, 3 + m, seed * 7 + 2)
    sp1 = [g1[i * pb1:(i + 1) * pb1] for i in range(len(g1) // pb1)]
    sp2 = [g2[i * 2 * pb1:(i + 1) * 2 * pb1] for i in range(len(g2) // (2 * pb1))]
    vk = dict(alpha_g1=sp1[0], beta_g1=sp1[1], delta_g1=sp1[2], beta_g2=sp2[0], gamma_g2=sp2[1], delta_g2=sp2[2])
    o = 5
    ic = sp1[o:o + num_public + 1]; o += num_public + 1
    a1 = sp1[o:o + m]; o += m
    b1 = sp1[o:o + m]; o += m
    c1 = sp1[o:o + m - num_public - 1]; o += m
    h1 = sp1[o:o + n]
    b2 = sp2[3:3 + m]
    # a couple of identity points in the queries (the zkey stores them as (0,0))
    if m > 3:
        a1[2] = b"\x00" * pb1
        b2[1] = b"\x00" * (2 * pb1)
    coefs = []
    for con in range(n):
        if rng.random() < empty_rows:
            continue
        for mat in (0, 1):
            for _ in range(rng.randint(1, nnz_per_row)):
                word = rng.randrange(r)
                coefs.append((mat, con, rng.randrange(m), word.to_bytes(n8r, "little")))
    rng.shuffle(coefs)
    if coefficients is not None:
        coefs = list(coefficients)
    overrides = full or {}
    full = [1] + [rng.randrange(r) for _ in range(m - 1)]
    if m > 4:
        full[3] = 0
    for sig, v in overrides.items():
        full[sig] = v
    z = write_zkey(curve, m, num_public, n, vk, ic, coefs, a1, b1, b2, c1, h1)
    return z, full


def random_r1cs(num_vars, num_public, num_constraints, terms, seed=1, no_a=(), no_b=(), unused=()):
    """A satisfied random R1CS over BN254 Fr: (rows, witness), rows a list of
    (A, B, C) with each side a {signal: coefficient} dict of up to `terms`
    terms, <A, w> <B, w> = <C, w> in every row.  Signals in `no_a` / `no_b`
    are in no A / B row, signals in `unused` in no row at all."""
    r = CURVE_FIELDS["bn254"][1]
    rng = random.Random(seed)
    w = [1] + [rng.randrange(1, r) for _ in range(num_vars - 1)]
    ok_a = [s for s in range(num_vars) if s not in no_a and s not in unused]
    ok_b = [s for s in range(num_vars) if s not in no_b and s not in unused]
    ok_c = [s for s in range(num_vars) if s not in unused]

    def side(pool):
        return {s: rng.randrange(1, r) for s in rng.sample(pool, min(terms, len(pool)))}

    def dot(row):
        return sum(c * w[s] for s, c in row.items()) % r

    rows = []
    for _ in range(num_constraints):
        A, B, C = side(ok_a), side(ok_b), side(ok_c)
        pivot = next(iter(C))  # C's first coefficient is set so that the row holds (every w[s] != 0)
        C[pivot] = 0
        C[pivot] = (dot(A) * dot(B) - dot(C)) * pow(w[pivot], -1, r) % r
        rows.append((A, B, C))
    return rows, w


def trapdoor_zkey(rows, num_vars, num_public, log_n=None, seed=1):
    """A verifiable BN254 proving key: snarkjs's Groth16 setup from a seeded
    trapdoor (tau, alpha, beta, gamma, delta) and the R1CS `rows` (a list of
    (A, B, C), each a {signal: coefficient} dict).  As snarkjs does, the rows
    A = x_i, B = 0 for the num_public + 1 instance signals follow the
    constraints.  With u_s, v_s, w_s the A / B / C column polynomials of signal
    s over the domain of size n (Lagrange basis L_j):
      a1[s] = [u_s(tau)]_1, b1[s] = [v_s(tau)]_1, b2[s] = [v_s(tau)]_2,
      ic[s] = [(beta u_s + alpha v_s + w_s)(tau) / gamma]_1 for the instance,
      c1[s] = [the same / delta]_1 for the witness signals,
      h1[i] = [L'_{2i+1}(tau) / delta]_1, L' the Lagrange basis of the domain of
        size 2n: the prover's h_i are the values of a b - c on the odd 2n-th
        roots, and a b - c vanishes on the even ones for a satisfying witness,
    and the coefficient words are c R^2 mod r (oracle.circom_format
    coefficient_value gives c back).  A signal in no A row (or no B row, or no
    row at all) gets the identity in a1 (b1 and b2, c1).  Returns zkey bytes."""
    G1, G2 = pyref.Curve("bn254_g1"), pyref.Curve("bn254_g2")
    Fr = G1.Fr
    r = Fr.p
    nrows = len(rows) + num_public + 1
    if log_n is None:
        log_n = max(1, (nrows - 1).bit_length())
    n = 1 << log_n
    assert nrows <= n
    rng = random.Random(seed)
    tau, alpha, beta, gamma, delta = (rng.randrange(2, r) for _ in range(5))

    def lagrange_at(size, x):  # L_j(x) = (x^size - 1) / size * w^j / (x - w^j)
        w = Fr.root_of_unity(size)
        z = (pow(x, size, r) - 1) * pow(size, -1, r) % r
        return [z * pow(w, j, r) * pow(x - pow(w, j, r), -1, r) % r for j in range(size)]

    L = lagrange_at(n, tau)
    a_rows = [A for A, _, _ in rows] + [{i: 1} for i in range(num_public + 1)]
    b_rows = [B for _, B, _ in rows] + [{} for _ in range(num_public + 1)]
    c_rows = [C for _, _, C in rows] + [{} for _ in range(num_public + 1)]
    u, v, w = [0] * num_vars, [0] * num_vars, [0] * num_vars
    for acc, side in ((u, a_rows), (v, b_rows), (w, c_rows)):
        for j, row in enumerate(side):
            for s, c in row.items():
                acc[s] = (acc[s] + c * L[j]) % r

    g1_gen, g2_gen = G1.to_bytes(G1.G), G2.to_bytes(G2.G)

    def g1(k):  # [k]_1 as affine Montgomery bytes (the C oracle's MSM over one point)
        return O.msm("bn254_g1", g1_gen, Fr.to_bytes(k))[0] if k % r else b"\x00" * 64

    def g2(k):
        return O.msm("bn254_g2", g2_gen, Fr.to_bytes(k))[0] if k % r else b"\x00" * 128

    inv_gamma, inv_delta = pow(gamma, -1, r), pow(delta, -1, r)
    k = [(beta * u[s] + alpha * v[s] + w[s]) % r for s in range(num_vars)]
    L2 = lagrange_at(2 * n, tau)
    vk = dict(alpha_g1=g1(alpha), beta_g1=g1(beta), delta_g1=g1(delta), beta_g2=g2(beta), gamma_g2=g2(gamma),
              delta_g2=g2(delta))
    R2 = (1 << 512) % r
    coefs = [(mat, j, s, (c * R2 % r).to_bytes(32, "little"))
             for mat, side in ((0, a_rows), (1, b_rows)) for j, row in enumerate(side) for s, c in row.items()]
    rng.shuffle(coefs)
    return write_zkey("bn254", num_vars, num_public, n, vk,
                      ic=[g1(k[s] * inv_gamma) for s in range(num_public + 1)], coefficients=coefs,
                      a1=[g1(x) for x in u], b1=[g1(x) for x in v], b2=[g2(x) for x in v],
                      c1=[g1(k[s] * inv_delta) for s in range(num_public + 1, num_vars)],
                      h1=[g1(L2[2 * i + 1] * inv_delta) for i in range(n)])


TRAPDOOR_SHAPE = dict(num_vars=16, num_public=4, num_constraints=11, terms=12, no_a=(5,), no_b=(6,), unused=(15,))


def trapdoor_fixture(seed=7):
    """The trapdoor key the CPU and GPU tests share: 16 signals (4 public), 11
    constraints of 12 terms a side plus the 5 instance rows = a full domain of
    16; signal 5 in no A row, 6 in no B row, witness signal 15 in no row.
    Returns (zkey bytes, witness)."""
    rows, w = random_r1cs(seed=seed, **TRAPDOOR_SHAPE)
    return trapdoor_zkey(rows, TRAPDOOR_SHAPE["num_vars"], TRAPDOOR_SHAPE["num_public"], seed=seed), w
