"""GPU Groth16 at its edges, through the C-ABI, bytewise against the CPU oracle
(oracle/groth16.py) on keys of at most 2^9 constraints:
  * a verifiable key larger than the reference's fixtures
    (groth16_synth.trapdoor_zkey: dense rows, a full domain, identity query
    points): the proofs equal the oracle's AND pass the pairing check for
    every zero / non-zero combination of the blinding factors, grouped and
    separate MSMs;
  * the witness map's row shapes: two workgroups of qap_abc_kernel, rows of
    0 .. 300 terms on one side with the other empty, a row naming one signal
    many times, the last constraint, the first and last signal, coefficient
    words at the edges of the Montgomery conversion (the value one among
    them), matrix 2 as B, witness values 0, 1 and r - 1, on both curves;
  * the smallest domains and a key with no query points at all;
  * one prover over many proofs (buffers that persist must not leak);
  * more shards than query points.
Witness bytes stay canonical (values >= r are outside the reference's
contract), and nothing here makes the C-ABI abort: malformed files are
tests/test_circom_io_check.py's, on the host.
"""
import random

import pytest

from oracle import bn254_pairing as BP
from oracle import circom_format as CF
from oracle import groth16 as OG
from oracle import pyref
from tachyon_amd import params as P

from groth16_synth import synth_zkey, trapdoor_fixture

pytestmark = pytest.mark.gpu
FR = {"bn254": pyref.Field("bn254_fr"), "bls12_381": pyref.Field("bls12_381_fr")}


def fr_bytes(curve, vals):
    return b"".join(FR[curve].to_bytes(v) for v in vals)


def word(v):
    return v.to_bytes(32, "little")


# ---- a verifiable key larger than the fixtures -------------------------------

@pytest.fixture(scope="module")
def trapdoor():
    zb, w = trapdoor_fixture()
    zk = CF.parse_zkey(zb)
    G1, G2 = pyref.Curve("bn254_g1"), pyref.Curve("bn254_g2")
    vk = {k: (G2 if k.endswith("g2") else G1).from_bytes(v) for k, v in zk["vk"].items()}
    ic = [G1.from_bytes(b) for b in zk["ic"]]
    h = OG.witness_map(zk, w)
    return dict(zb=zb, zk=zk, w=w, h=h, vk=vk, ic=ic, G1=G1, G2=G2)


def test_trapdoor_witness_map(trapdoor):
    from tachyon_amd.groth16 import Groth16Prover
    prover = Groth16Prover(trapdoor["zb"])
    assert (prover.num_vars, prover.num_public, prover.domain_size) == (16, 4, 16)
    assert prover.witness_map(fr_bytes("bn254", trapdoor["w"])) == fr_bytes("bn254", trapdoor["h"])
    prover.close()


@pytest.mark.parametrize("r_blind,s_blind", [(0, 0), (0x5EED, 0), (0, P.BN254_FR - 3), (0xC0FFEE, P.BN254_FR - 9)])
def test_trapdoor_proofs_equal_the_oracle_and_verify(trapdoor, r_blind, s_blind):
    from tachyon_amd.groth16 import Groth16Prover
    t = trapdoor
    G1, G2, Fr = t["G1"], t["G2"], FR["bn254"]
    want = OG.prove(t["zk"], t["w"], r_blind, s_blind, h=t["h"])
    fb = fr_bytes("bn254", t["w"])
    prover = Groth16Prover(t["zb"])
    verified = {}  # (the pairing check is a function of the proof bytes: once per distinct proof)
    for variant in (0, 1):
        prover.set_variant(variant)
        got = prover.prove(fb) if (r_blind, s_blind) == (0, 0) else \
            prover.prove(fb, Fr.to_bytes(r_blind), Fr.to_bytes(s_blind))
        assert tuple(got) == tuple(want), variant
        if got not in verified:
            A, B, C = got
            verified[got] = BP.groth16_verify(t["vk"], t["ic"], t["w"][1:5],
                                              (G1.from_bytes(A), G2.from_bytes(B), G1.from_bytes(C)))
        assert verified[got], variant
    prover.close()


# ---- row shapes -----------------------------------------------------------------

ROW_TERMS = (0, 1, 2, 63, 64, 65, 300)


def edge_words(r):
    """Coefficient words at the edges of word * R^-2 mod r: zero, the value one
    (R^2 mod r; the reference special-cases it), the words around r, 2^256 - 1."""
    return [0, (1 << 512) % r, r - 1, r, r + 1, (1 << 256) - 1]


def row_shape_key(curve):
    r = FR[curve].p
    log_n, m = 9, 320
    n = 1 << log_n
    rng = random.Random(909)
    coefs = []

    def terms(mat, con, signals, words=None):
        for i, s in enumerate(signals):
            coefs.append((mat, con, s, word(words[i] if words else rng.randrange(r))))

    # one side of 0 .. 300 terms, the other empty -- in both workgroups of qap_abc_kernel (256 rows each)
    for base in (0, 256):
        for i, k in enumerate(ROW_TERMS):
            terms(0, base + 3 * i, rng.sample(range(m), k))
            terms(1, base + 3 * i + 1, rng.sample(range(m), k))
    terms(0, 40, [17] * 5)  # every term names one signal
    terms(1, 40, [17] * 3 + [18])
    terms(0, 41, [0, m - 1])  # the first and the last signal
    terms(1, 41, [m - 1, 0])
    terms(0, n - 1, [1, 2])  # the last constraint
    terms(1, n - 1, [3, m - 1])
    ew = edge_words(r)
    for i, w in enumerate(ew):  # every edge word on each side, against the value one and against itself
        terms(0, 50 + i, [100 + i % 3], [w])
        terms(1, 50 + i, [101 + i % 3], [ew[1]])
        terms(0, 60 + i, [102], [ew[1]])
        terms(1, 60 + i, [100 + i % 3, 5], [w, w])
    terms(0, 70, [3])
    terms(2, 70, [4])  # matrix 2 is B
    terms(0, 80, [100, 101, 102])  # the witness values 0, 1 and r - 1
    terms(1, 80, [102, 101, 100])
    for con in list(range(90, 256)) + list(range(290, n - 1)):
        if rng.random() < 0.1:
            continue
        terms(0, con, rng.choices(range(m), k=rng.randint(1, 3)))
        terms(1, con, rng.choices(range(m), k=rng.randint(1, 3)))
    rng.shuffle(coefs)
    return synth_zkey(curve, log_n=log_n, num_vars=m, num_public=2, seed=77, coefficients=coefs,
                      full={100: 0, 101: 1, 102: r - 1, m - 1: r - 1})


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_row_shapes(curve):
    from tachyon_amd.groth16 import Groth16Prover
    zbytes, full = row_shape_key(curve)
    zk = CF.parse_zkey(zbytes)
    assert zk["domain_size"] == 512 and sum(1 for c in zk["coefficients"] if c[0] == 2) == 1
    rows = {}
    for mat, con, _, _ in zk["coefficients"]:
        rows[(min(mat, 1), con)] = rows.get((min(mat, 1), con), 0) + 1
    for base in (0, 256):  # (the shapes the test is about are in the key)
        assert [rows.get((0, base + 3 * i), 0) for i in range(7)] == list(ROW_TERMS)
        assert [rows.get((1, base + 3 * i), 0) for i in range(7)] == [0] * 7
        assert [rows.get((1, base + 3 * i + 1), 0) for i in range(7)] == list(ROW_TERMS)
    Fr = FR[curve]
    fb = fr_bytes(curve, full)
    h = OG.witness_map(zk, full)
    prover = Groth16Prover(zbytes)
    assert prover.witness_map(fb) == fr_bytes(curve, h)
    want = list(OG.prove(zk, full, h=h))
    assert list(prover.prove(fb)) == want
    r, s = 0xED6E5, Fr.p - 0xED6E
    assert list(prover.prove(fb, Fr.to_bytes(r), Fr.to_bytes(s))) == list(OG.prove(zk, full, r, s, h=h))
    prover.set_variant(1)
    assert list(prover.prove(fb)) == want
    prover.close()


# ---- smallest shapes --------------------------------------------------------------

@pytest.mark.parametrize("log_n,num_vars,num_public", [(1, 4, 2), (2, 4, 2), (1, 1, 0), (2, 1, 0)])
def test_smallest_shapes(log_n, num_vars, num_public):
    """Domains of 2 and 4 rows; num_vars = 1: every query MSM is empty and the
    proof is the key's constant terms plus the h MSM."""
    from tachyon_amd.groth16 import Groth16Prover
    zbytes, full = synth_zkey("bn254", log_n=log_n, num_vars=num_vars, num_public=num_public, seed=50 + log_n,
                              empty_rows=0.0)
    zk = CF.parse_zkey(zbytes)
    assert zk["domain_size"] == 1 << log_n and len(zk["a1"]) == num_vars and len(zk["c1"]) == num_vars - num_public - 1
    Fr = FR["bn254"]
    fb = fr_bytes("bn254", full)
    h = OG.witness_map(zk, full)
    prover = Groth16Prover(zbytes)
    assert prover.witness_map(fb) == fr_bytes("bn254", h)
    r, s = 0x51A11, Fr.p - 2
    for variant in (0, 1):
        prover.set_variant(variant)
        assert list(prover.prove(fb)) == list(OG.prove(zk, full, h=h)), variant
        assert list(prover.prove(fb, Fr.to_bytes(r), Fr.to_bytes(s))) == list(OG.prove(zk, full, r, s, h=h)), variant
    prover.close()


# ---- one prover, many proofs ----------------------------------------------------------

def test_one_prover_many_proofs():
    """Witnesses, blinding factors, variants and window bits change between the
    proofs of one prover: the scalar staging, the grouped layout's padding
    and the fold tables persist across them and must not leak from one proof
    into the next."""
    from tachyon_amd.groth16 import Groth16Prover
    zbytes, w1 = synth_zkey("bn254", log_n=6, seed=21)
    zk = CF.parse_zkey(zbytes)
    Fr = FR["bn254"]
    m = zk["num_vars"]
    rng = random.Random(22)
    w2 = [1] + [rng.randrange(Fr.p) for _ in range(m - 1)]
    unit = [1] + [0] * (m - 1)
    b1, b2, bu = (fr_bytes("bn254", w) for w in (w1, w2, unit))
    r, s = 0xFACADE, Fr.p - 0xBEE
    rb, sb, zero = Fr.to_bytes(r), Fr.to_bytes(s), Fr.to_bytes(0)
    h1 = OG.witness_map(zk, w1)
    prover = Groth16Prover(zbytes)
    assert list(prover.prove(b1)) == list(OG.prove(zk, w1, h=h1))
    assert list(prover.prove(b2)) == list(OG.prove(zk, w2))
    assert prover.witness_map(b1) == fr_bytes("bn254", h1)
    assert list(prover.prove(bu)) == list(OG.prove(zk, unit))
    prover.set_variant(1)
    assert list(prover.prove(b2)) == list(OG.prove(zk, w2))
    prover.set_variant(0)
    assert list(prover.prove(b1, rb, sb)) == list(OG.prove(zk, w1, r, s, h=h1))
    prover.set_msm_window_bits(5, 6, 7)
    assert list(prover.prove(b2, rb, zero)) == list(OG.prove(zk, w2, r, 0))
    assert list(prover.prove(b1, zero, sb)) == list(OG.prove(zk, w1, 0, s, h=h1))
    prover.close()


# ---- shards past the query length ---------------------------------------------------------

@pytest.mark.parametrize("with_b1", [True, False])
def test_more_shards_than_query_points(with_b1):
    """num_vars = 4 over world = 8: three query points and five witness + h
    points, so most ranks hold an empty shard of one MSM or of all of them.
    The assembled proof equals prove() and the oracle's."""
    from tachyon_amd.groth16 import Groth16Prover
    world = 8
    zbytes, full = synth_zkey("bn254", log_n=2, num_vars=4, num_public=2, seed=61, empty_rows=0.0)
    zk = CF.parse_zkey(zbytes)
    Fr = FR["bn254"]
    fb = fr_bytes("bn254", full)
    r, s = (0xB1B1 if with_b1 else 0), Fr.p - 0x5A
    rb, sb = Fr.to_bytes(r), Fr.to_bytes(s)
    prover = Groth16Prover(zbytes)
    parts = [prover.prove_partials(fb, k, world, with_b1=with_b1) for k in range(world)]
    blob = b"".join(parts)
    want_nozk, want_zk = list(OG.prove(zk, full)), list(OG.prove(zk, full, r, s))
    assert list(prover.assemble(blob)) == want_nozk == list(prover.prove(fb))
    assert list(prover.assemble(blob, rb, sb)) == want_zk == list(prover.prove(fb, rb, sb))
    prover.close()
