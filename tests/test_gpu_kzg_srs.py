"""The KZG SRS and its commitments where tests/test_gpu_kzg.py does not reach:
SRS sizes of one element, two, one full workgroup of srs_scalars_kernel /
fixed_base_kernel and a second one, against tests/kzg_ref.py; trapdoors 0, 1, 2,
r - 1 and w^(n-1) (the ends and the middle of the host's search for w^j = tau);
identities that need no oracle, among them commitments that are the point at
infinity with no zero scalar; the whole API on BLS12-381; identities at every
place of a batch normalised with one inversion; and one handle set up again and
again.  Everything is bytewise equality."""
import functools

import pytest

import kzg_ref as K
from oracle import oracle as O
from oracle import pyref

pytestmark = pytest.mark.gpu

CURVES = ["bn254_g1", "bls12_381_g1"]
TAU0 = 0x1234_5678_9ABC_DEF0


def scalar_field(curve):
    return pyref.Field(K.SCALAR_FIELD[curve])


def trapdoor(curve, n, name):
    Fr = scalar_field(curve)
    if name == "r-1":
        return Fr.p - 1
    if name == "w^(n-1)":
        return pow(Fr.root_of_unity(n), n - 1, Fr.p)
    return int(name, 0)


@functools.lru_cache(maxsize=None)
def ref_srs(curve, n, tau):
    """(tau^i, L_i(tau), [tau^i]G, [L_i(tau)]G) of the reference, computed once."""
    s, l = K.srs_scalars(K.SCALAR_FIELD[curve], n, tau)
    return s, l, K.srs_points(curve, s), K.srs_points(curve, l)


def to_bytes(curve, ints):
    Fr = scalar_field(curve)
    return b"".join(Fr.to_bytes(v) for v in ints)


def seeded(curve, seed, n):
    return O.gen_scalars(K.SCALAR_FIELD[curve], seed, n).tobytes()


def generator(curve):
    C = pyref.Curve(curve)
    return C.to_bytes(C.G)


def new_kzg(curve, n, tau):
    from tachyon_amd.kzg import KZG
    kzg = KZG(curve)
    kzg.unsafe_setup(n, None if tau is None else scalar_field(curve).to_bytes(tau))
    return kzg


def points(kzg, raw):
    pb = kzg.point_bytes
    assert len(raw) % pb == 0
    return [raw[i:i + pb] for i in range(0, len(raw), pb)]


def first_difference(got, want, pb):
    """None, or the index of the first point that differs (for the message)."""
    if got == want:
        return None
    if len(got) != len(want):
        return "length %d != %d" % (len(got), len(want))
    return next(i for i in range(len(got) // pb) if got[i * pb:(i + 1) * pb] != want[i * pb:(i + 1) * pb])


def check_srs(kzg, curve, n, tau, keep=None):
    """N() and both read-backs against the reference; keep: the prefix a
    downsize left."""
    keep = n if keep is None else keep
    pb = kzg.point_bytes
    _, _, powers, lag = ref_srs(curve, n, tau)
    assert kzg.N() == keep
    assert first_difference(kzg.g1_powers_of_tau(), powers[:keep * pb], pb) is None
    assert first_difference(kzg.g1_powers_of_tau_lagrange(), lag[:keep * pb], pb) is None
    return powers[:keep * pb], lag[:keep * pb]


def check_full_commit(kzg, curve, powers, lag, seed):
    """A commitment of N scalars on each SRS vector against the oracle's MSM."""
    v = seeded(curve, seed, kzg.N())
    assert kzg.commit(v) == O.msm(curve, powers, v)[0]
    assert kzg.commit_lagrange(v) == O.msm(curve, lag, v)[0]


def check_oracle_free(kzg, curve, n, tau, seed):
    """What holds for any trapdoor: powers[0] = G, sum L_i = 1, sum w^i L_i =
    tau, Commit(p) = CommitLagrange(FFT(p)); and for a known one, the two
    commitments to x - tau are the identity."""
    Fr = scalar_field(curve)
    r, w = Fr.p, Fr.root_of_unity(n)
    G, pb = generator(curve), kzg.point_bytes
    powers = points(kzg, kzg.g1_powers_of_tau())
    assert kzg.N() == n and len(powers) == n and len(kzg.g1_powers_of_tau_lagrange()) == n * pb
    assert powers[0] == G
    assert kzg.commit_lagrange(to_bytes(curve, [1] * n)) == G
    domain = [pow(w, i, r) for i in range(n)]
    assert kzg.commit_lagrange(to_bytes(curve, domain)) == powers[1]
    p = seeded(curve, seed, n)
    c = kzg.commit(p)
    assert c == kzg.commit_lagrange(O.fft(p, n, field=Fr.name))
    assert c != bytes(pb) and O.ec_op(curve, "on_curve", c)
    if tau is not None:
        assert kzg.commit(to_bytes(curve, [r - tau, 1])) == bytes(pb)
        assert kzg.commit_lagrange(to_bytes(curve, [(x - tau) % r for x in domain])) == bytes(pb)


# ------------------------------------------------------ SRS against the reference

@pytest.mark.parametrize("n", [1, 2, 256, 512])
@pytest.mark.parametrize("curve", CURVES)
def test_srs_against_reference(curve, n):
    """Sizes up to and past one workgroup of 256: an element at i >= 256 with
    the wrong block index, exponent or domain root differs from the reference,
    as does the root of the one- and two-element domains."""
    tau = TAU0 + n
    kzg = new_kzg(curve, n, tau)
    powers, lag = check_srs(kzg, curve, n, tau)
    s, l, _, _ = ref_srs(curve, n, tau)
    idx = sorted({i for i in (0, 1, 255, 256, n - 1) if i < n})
    got_p, got_l = points(kzg, kzg.g1_powers_of_tau()), points(kzg, kzg.g1_powers_of_tau_lagrange())
    for i, pt in K.spot_points(curve, s, idx).items():
        assert got_p[i] == pt, i
    for i, pt in K.spot_points(curve, l, idx).items():
        assert got_l[i] == pt, i
    check_full_commit(kzg, curve, powers, lag, 40 + n)
    kzg.close()


# ----------------------------------------------------------------- trapdoor edges

EDGES = [(512, t) for t in ("0", "1", "2", "r-1", "w^(n-1)")] + [(2, t) for t in ("0", "1", "2", "r-1")]


@pytest.mark.parametrize("n,tau_name", EDGES, ids=["%d-%s" % e for e in EDGES])
@pytest.mark.parametrize("curve", CURVES)
def test_trapdoor_edges(curve, n, tau_name):
    """tau = 0: G then identities, every Lagrange point [1/n]G.  tau = 2: the
    single-bit scalars 2^i up to 2^511 mod r.  tau = 1, r - 1, w^(n-1): the
    host's search for w^j = tau ends at j = 0, n/2, n - 1 (for n = 2, w = r - 1)."""
    Fr = scalar_field(curve)
    tau = trapdoor(curve, n, tau_name)
    kzg = new_kzg(curve, n, tau)
    powers, lag = check_srs(kzg, curve, n, tau)
    G, pb = generator(curve), kzg.point_bytes
    if tau_name == "0":
        assert powers == G + bytes(pb * (n - 1))
        inv_n = O.ec_op(curve, "mul", G, pow(n, -1, Fr.p).to_bytes(32, "little"))
        assert lag == inv_n * n
    in_domain = {"1": 0, "r-1": n // 2, "w^(n-1)": n - 1}
    if tau_name in in_domain:
        j = in_domain[tau_name]
        assert lag == bytes(pb * j) + G + bytes(pb * (n - 1 - j))
    check_full_commit(kzg, curve, powers, lag, 60 + n)
    kzg.close()


# ------------------------------------------------- answers that need no oracle

@pytest.mark.parametrize("fixed", [False, True], ids=["random_tau", "fixed_tau"])
@pytest.mark.parametrize("curve", CURVES)
def test_oracle_free_identities(curve, fixed):
    """commit([r - tau, 1]) and commit_lagrange([w^i - tau]) are the identity
    although no scalar is zero: the sum cancels only in the last addition of
    the window sums."""
    n = 512
    tau = TAU0 + n if fixed else None
    kzg = new_kzg(curve, n, tau)
    check_oracle_free(kzg, curve, n, tau, 70)
    kzg.close()


# ----------------------------------------------- the whole API on both curves

@pytest.mark.parametrize("curve", CURVES)
def test_batch_and_downsize(curve):
    n = 64
    tau = TAU0 + n
    Fr = scalar_field(curve)
    kzg = new_kzg(curve, n, tau)
    powers, lag_srs = check_srs(kzg, curve, n, tau)
    pb = kzg.point_bytes
    polys = [seeded(curve, 900 + i, n) for i in range(10)]
    evals = [O.fft(p, n, field=Fr.name) for p in polys]
    batch = kzg.commit_batch(polys)
    lag = kzg.commit_batch(evals, lagrange=True)
    assert batch == [O.msm(curve, powers, p)[0] for p in polys]
    assert lag == [O.msm(curve, lag_srs, e)[0] for e in evals]
    assert batch == lag == [kzg.commit(p) for p in polys]
    # ragged batch with an empty and a zero polynomial
    ragged = [polys[0][:32 * 3], b"", bytes(32 * n), polys[1]]
    got = kzg.commit_batch(ragged)
    assert got == [O.msm(curve, powers[:len(p) // 32 * pb], p)[0] if p else bytes(pb) for p in ragged]
    assert got == [kzg.commit(p) if p else bytes(pb) for p in ragged]
    assert got[1] == bytes(pb) and got[2] == bytes(pb)
    assert kzg.commit_batch([polys[0] + polys[0][:32]]) is None  # more than N: nothing written
    assert kzg.commit_batch([polys[1], polys[0] + polys[0][:32]], lagrange=True) is None
    assert kzg.commit_batch([]) == []
    assert not kzg.downsize(n) and not kzg.downsize(n + 1) and kzg.N() == n
    assert kzg.downsize(n // 2) and kzg.N() == n // 2
    check_srs(kzg, curve, n, tau, keep=n // 2)
    # more scalars than N: the reference's Commit / CommitLagrange return false
    assert kzg.commit(polys[0]) is None and kzg.commit_lagrange(polys[0]) is None
    assert kzg.commit_batch([polys[0]]) is None
    half = polys[0][:32 * (n // 2)]
    assert kzg.commit(half) == O.msm(curve, powers[:n // 2 * pb], half)[0]
    assert kzg.commit_lagrange(half) == O.msm(curve, lag_srs[:n // 2 * pb], half)[0]
    kzg.close()


@pytest.mark.parametrize("curve", CURVES)
def test_device_resident_scalars(curve):
    import numpy as np
    import torch
    n = 64
    tau = TAU0 + n
    kzg = new_kzg(curve, n, tau)
    _, _, powers, lag = ref_srs(curve, n, tau)
    coeffs = O.gen_scalars(K.SCALAR_FIELD[curve], 7, n)
    d = torch.from_numpy(coeffs.view(np.uint8).copy()).cuda()
    host = kzg.commit(coeffs.tobytes())
    assert host == O.msm(curve, powers, coeffs.tobytes())[0]
    assert kzg.commit(d) == host
    assert kzg.commit_lagrange(d) == kzg.commit_lagrange(coeffs.tobytes()) == O.msm(curve, lag, coeffs.tobytes())[0]
    assert kzg.commit_batch([d, coeffs.tobytes()[:32 * 5], d]) == [host, kzg.commit(coeffs.tobytes()[:32 * 5]), host]
    kzg.close()


# ------------------------------------------------------ batch normalisation edges

# Z the zero polynomial, E the empty one, m = -p, X = [r - tau, 1]
BATCHES = ["Z", "E", "ZEZ", "Zpq", "pqZ", "p", "pm", "pXq"]


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("curve", CURVES)
def test_batch_normalisation_edges(curve, batch):
    """Identities first, last, alone and everywhere in the batch whose ZZZ are
    inverted together; X = [r - tau, 1] is an identity that the MSM, not a zero
    scalar, produces; p and -p share x and have opposite y."""
    n = 8
    tau = TAU0 + n
    Fr = scalar_field(curve)
    r = Fr.p
    kzg = new_kzg(curve, n, tau)
    powers, lag_srs = check_srs(kzg, curve, n, tau)
    pb = kzg.point_bytes
    p_int = pyref.gen_scalars(Fr, 21, n)
    poly = {
        "Z": bytes(32 * n),
        "E": b"",
        "p": to_bytes(curve, p_int),
        "q": seeded(curve, 22, n - 3),
        "m": to_bytes(curve, [(r - v) % r for v in p_int]),
        "X": to_bytes(curve, [r - tau, 1]),
    }
    polys = [poly[ch] for ch in batch]
    for lagrange, srs in ((False, powers), (True, lag_srs)):
        one = kzg.commit_lagrange if lagrange else kzg.commit
        got = kzg.commit_batch(polys, lagrange=lagrange)
        want = [O.msm(curve, srs[:len(v) // 32 * pb], v)[0] if v else bytes(pb) for v in polys]
        assert got == want
        assert got == [one(v) for v in polys]
        for ch, c in zip(batch, got):
            assert (c == bytes(pb)) == (ch in "ZE" or (ch == "X" and not lagrange)), ch
        if batch == "pm":
            assert O.ec_op(curve, "add", got[0], got[1]) == bytes(pb)
            half = pb // 2
            assert got[0][:half] == got[1][:half] and got[0][half:] != got[1][half:]
    kzg.close()


@pytest.mark.parametrize("curve", CURVES)
def test_empty_commit(curve):
    kzg = new_kzg(curve, 8, TAU0 + 8)
    assert kzg.commit(b"") == bytes(kzg.point_bytes)
    assert kzg.commit_lagrange(b"") == bytes(kzg.point_bytes)
    kzg.close()


# ------------------------------------------------------ one handle, several setups

@pytest.mark.parametrize("curve", CURVES)
def test_one_handle_several_setups(curve):
    """512, 8, downsize(4), 1024, 2 on one handle: the buffers keep their
    capacity, so a stale N or a stale element of an earlier, larger SRS shows
    in the read-backs or in a commitment of N scalars.  Every step has its own
    trapdoor."""
    Fr = scalar_field(curve)
    kzg = new_kzg(curve, 512, TAU0 + 512)
    powers, lag = check_srs(kzg, curve, 512, TAU0 + 512)
    check_full_commit(kzg, curve, powers, lag, 81)

    kzg.unsafe_setup(8, Fr.to_bytes(TAU0 + 8))
    powers, lag = check_srs(kzg, curve, 8, TAU0 + 8)
    check_full_commit(kzg, curve, powers, lag, 82)

    assert kzg.downsize(4)
    powers, lag = check_srs(kzg, curve, 8, TAU0 + 8, keep=4)
    check_full_commit(kzg, curve, powers, lag, 83)
    assert kzg.commit(seeded(curve, 83, 5)) is None

    tau = TAU0 + 1024
    kzg.unsafe_setup(1024, Fr.to_bytes(tau))
    check_oracle_free(kzg, curve, 1024, tau, 84)
    s, l = K.srs_scalars(Fr.name, 1024, tau)
    got_p, got_l = points(kzg, kzg.g1_powers_of_tau()), points(kzg, kzg.g1_powers_of_tau_lagrange())
    idx = [1, 255, 256, 512, 1023]  # a few elements of the largest size against the reference too
    assert b"".join(got_p[i] for i in idx) == K.srs_points(curve, [s[i] for i in idx])
    assert b"".join(got_l[i] for i in idx) == K.srs_points(curve, [l[i] for i in idx])
    check_full_commit(kzg, curve, b"".join(got_p), b"".join(got_l), 85)

    kzg.unsafe_setup(2, Fr.to_bytes(TAU0 + 2))
    powers, lag = check_srs(kzg, curve, 2, TAU0 + 2)
    check_full_commit(kzg, curve, powers, lag, 86)
    assert kzg.commit(seeded(curve, 86, 3)) is None
    kzg.close()
