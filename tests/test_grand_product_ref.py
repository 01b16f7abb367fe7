"""The grand-product reference module on the CPU (tests/grand_product_ref.py)
and the refusals of tachyon_mi355x_grand_product_chains, which are decided
before any GPU call.

The permutation argument's own identity checks the reference on the golden
circuits' sigma columns (tests/golden/halo2_circuits.json): a witness that is
constant on every cycle of the permutation gives a final chain value of 1 for
any chunk length, and one changed cell does not.
"""
import ctypes

import pytest

import grand_product_ref as R
import halo2_golden as H
from oracle import pyref

F = H.FR
DELTA = R.get_delta(F)
PERM_CASES = [c for c in H.circuits() if c.get("permutations_columns")]
PERM_IDS = [H.case_id(c) for c in PERM_CASES]


def fr(x):
    return F.to_bytes(x)


def rand(seed, count):
    return [pyref.rand_scalar(seed, i, F.p) for i in range(count)]


def perm_setup(c):
    n, omega = c["n"], int(c["omega"], 16)
    sig = [[int(h, 16) for h in col] for col in c["permutations_columns"]]
    return n, omega, sig, H.indicator_polys(c)["u"]


def test_the_five_permutation_circuits_are_there():
    assert PERM_IDS == ["simple_circuit#0", "simple_circuit#1", "fibonacci1_circuit#0", "fibonacci1_circuit#1",
                        "fibonacci2_circuit#0"]
    assert DELTA == pow(7, 1 << 28, F.p)
    assert pow(DELTA, (F.p - 1) >> 28, F.p) == 1 and DELTA != 1  # order divides the odd part T


@pytest.mark.parametrize("c", PERM_CASES, ids=PERM_IDS)
def test_sigma_values_are_labels_and_a_permutation(c):
    n, omega, sig, u = perm_setup(c)
    assert u == 10
    assert pow(omega, n, F.p) == 1 and pow(omega, n // 2, F.p) != 1
    cells = R.decode_sigmas(F, sig, omega, DELTA)  # KeyError: a value that is no label
    flat = [cell for col in cells for cell in col]
    assert sorted(flat) == [(i, j) for i in range(len(sig)) for j in range(n)]


@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("c", PERM_CASES, ids=PERM_IDS)
def test_cycle_constant_witness_closes_the_chain(c, L):
    n, omega, sig, u = perm_setup(c)
    cells = R.decode_sigmas(F, sig, omega, DELTA)
    w = R.cycle_constant_witness(F, cells, 900 + L)
    sigmas = [R.encode(F, col) for col in sig]
    beta, gamma = fr(0xBE7A), fr(0x6A33A)
    jobs = -(-len(sig) // L)
    blinds = [rand(50 + k, n - u - 1) for k in range(jobs)]

    def last_of(witness):
        chains = R.permutation_chains([[R.encode(F, col) for col in witness]], sigmas, beta, gamma, L + 2)
        assert [len(ch) for ch in chains] == [jobs]
        z, last = R.grand_product_chains(F, n, u, chains, omega, DELTA, blinds)
        return z, F.from_bytes(last[0])

    z, last = last_of(w)
    assert last == 1
    assert len(z) == jobs and all(len(zz) == 32 * n for zz in z)
    # one cell of a cycle longer than one changed: the product no longer closes
    i, j = next(cyc[0] for cyc in R.cycles(cells) if len(cyc) > 1 and all(r < u for _, r in cyc))
    bad = [list(col) for col in w]
    bad[i][j] = (bad[i][j] + 1) % F.p
    assert last_of(bad)[1] != 1


def small_chain(n, seed, jobs=3):
    cols = [R.encode(F, rand(seed + k, n)) for k in range(2 * jobs)]
    return [[([R.factor(cols[2 * k], c=fr(3 + k))], [R.factor(cols[2 * k + 1], m=fr(5), table=cols[2 * k], c=fr(7))])
             for k in range(jobs)]], cols


def test_chain_rule_and_blinds():
    n, u = 12, 7
    chains, _ = small_chain(n, 10)
    blinds = [rand(70 + k, n - u - 1) for k in range(3)]
    z, last = R.grand_product_chains(F, n, u, chains, 1, 1, blinds)
    rows = [R.decode(F, zz) for zz in z]
    assert rows[0][0] == 1
    for k in range(1, 3):
        assert rows[k][0] == rows[k - 1][u]
    assert F.from_bytes(last[0]) == rows[2][u]
    for k in range(3):
        assert rows[k][u + 1:] == blinds[k]  # rows u+1 .. n-1 only
        num, den = chains[0][k]
        a = R.decode(F, num[0]["values"])
        b = R.decode(F, den[0]["values"])
        for j in range(u):  # the recurrence, multiplied out
            lhs = rows[k][j + 1] * ((b[j] + 5 * a[j] + 7) % F.p) % F.p
            assert lhs == rows[k][j] * ((a[j] + 3 + k) % F.p) % F.p
    # u = 0: z = [z0, blinds...]
    z0, last0 = R.grand_product_chains(F, 4, 0, [[small_chain(4, 20, jobs=1)[0][0][0]]], 1, 1, [[9, 8, 7]])
    assert z0[0][:32] == fr(1) and R.decode(F, z0[0])[1:] == [9, 8, 7] and last0 == [fr(1)]


def test_zero_denominator_gives_zero_from_there_on():
    n, u, at = 12, 9, 4
    a = rand(1, n)
    s = rand(2, n)
    beta, gamma = 11, 13
    v = list(a)
    v[at] = (-beta * s[at] - gamma) % F.p  # v + beta sigma + gamma = 0 at row `at`
    job0 = ([R.factor(R.encode(F, a), c=fr(1))], [R.factor(R.encode(F, v), m=fr(beta), table=R.encode(F, s), c=fr(gamma))])
    job1 = ([R.factor(R.encode(F, a), c=fr(2))], [R.factor(R.encode(F, s), c=fr(3))])
    z, last = R.grand_product_chains(F, n, u, [[job0, job1]], 1, 1, [[5, 6]] * 2)
    r0, r1 = R.decode(F, z[0]), R.decode(F, z[1])
    assert all(x != 0 for x in r0[:at + 1])
    assert r0[at + 1:u + 1] == [0] * (u - at)
    assert r1[:u + 1] == [0] * (u + 1) and last == [fr(0)]
    assert r0[u + 1:] == [5, 6] and r1[u + 1:] == [5, 6]


def test_label_factor_is_delta_i_omega_j():
    n, u = 8, 5
    omega = F.root_of_unity(n)
    v = rand(3, n)
    ones = R.encode(F, [1] * n)
    lab = [pow(DELTA, 3, F.p) * pow(omega, j, F.p) % F.p for j in range(n)]
    by_label = ([R.factor(R.encode(F, v), m=fr(21), label=3, c=fr(4))], [R.factor(ones)])
    by_table = ([R.factor(R.encode(F, v), m=fr(21), table=R.encode(F, lab), c=fr(4))], [R.factor(ones)])
    bl = [[0, 0]]
    assert R.grand_product_chains(F, n, u, [[by_label]], omega, DELTA, bl) == \
        R.grand_product_chains(F, n, u, [[by_table]], omega, DELTA, bl)


def test_lookup_and_shuffle_callbacks():
    n, u = 8, 6
    A, S = rand(4, n), rand(5, n)
    Ap, Sp = rand(6, n), rand(7, n)
    enc = [R.encode(F, x) for x in (A, S, Ap, Sp)]
    z, _ = R.grand_product_chains(F, n, u, [[R.lookup_job(*enc, fr(17), fr(19))]], 1, 1, [[1]])
    row = R.decode(F, z[0])
    for j in range(u):
        assert row[j + 1] * (Ap[j] + 17) * (Sp[j] + 19) % F.p == row[j] * (A[j] + 17) * (S[j] + 19) % F.p
    z, _ = R.grand_product_chains(F, n, u, [[R.shuffle_job(enc[0], enc[1], fr(23))]], 1, 1, [[1]])
    row = R.decode(F, z[0])
    for j in range(u):
        assert row[j + 1] * (S[j] + 23) % F.p == row[j] * (A[j] + 23) % F.p


# --- the library's refusals (no GPU call is made) ------------------------------
SENTINEL = 0xA5


class Call:
    """A valid call of one chain of one job (one factor each side, a label
    factor in the numerator) whose parts a test then damages."""

    def __init__(self, n=8, u=5):
        from tachyon_amd.plonk import GpFactor, GpPoly
        self.n, self.u, self.field = n, u, 0
        self.values = ctypes.create_string_buffer(R.encode(F, rand(40, n)), 32 * n)
        self.table = ctypes.create_string_buffer(R.encode(F, rand(41, n)), 32 * n)
        self.num = (GpFactor * 1)()
        self.den = (GpFactor * 1)()
        self.num[0].values = ctypes.addressof(self.values)
        self.num[0].kind, self.num[0].label = 2, 1
        self.den[0].values = ctypes.addressof(self.values)
        self.den[0].table = ctypes.addressof(self.table)
        self.den[0].kind = 1
        self.polys = (GpPoly * 1)()
        self.polys[0].num, self.polys[0].num_count = self.num, 1
        self.polys[0].den, self.polys[0].den_count = self.den, 1
        self.lens = (ctypes.c_size_t * 1)(1)
        self.num_chains = 1
        self.omega = ctypes.create_string_buffer(fr(F.root_of_unity(n)), 32)
        self.delta = ctypes.create_string_buffer(fr(DELTA), 32)
        self.blinds = ctypes.create_string_buffer(R.encode(F, rand(42, n - u - 1)), 32 * (n - u - 1))
        self.z = ctypes.create_string_buffer(bytes([SENTINEL]) * (32 * n), 32 * n)
        self.outs = (ctypes.c_void_p * 1)(ctypes.addressof(self.z))
        self.last = ctypes.create_string_buffer(bytes([SENTINEL]) * 32, 32)
        self.polys_arg, self.lens_arg, self.outs_arg = self.polys, self.lens, self.outs

    def run(self):
        from tachyon_amd._lib import lib
        return lib().tachyon_mi355x_grand_product_chains(self.field, self.n, self.u, self.omega, self.delta,
                                                         self.polys_arg, self.lens_arg, self.num_chains, self.blinds,
                                                         self.outs_arg, self.last)

    def untouched(self):
        return self.z.raw == bytes([SENTINEL]) * len(self.z.raw) and len(self.z.raw) == 256 and self.last.raw == bytes([SENTINEL]) * 32


def _set(name, value):
    def f(c):
        setattr(c, name, value)
    return f


def _no_values(c):
    c.num[0].values = None


def _bad_kind(c):
    c.num[0].kind = 3


def _no_table(c):
    c.den[0].table = None


def _no_factors(c):
    c.polys[0].num_count = c.polys[0].den_count = 0


def _null_num(c):
    c.polys[0].num = ctypes.POINTER(type(c.num[0]))()


def _null_den(c):
    c.polys[0].den = ctypes.POINTER(type(c.den[0]))()


REFUSALS = {
    "null polys": _set("polys_arg", None),
    "null chain_lens": _set("lens_arg", None),
    "null numerator list": _null_num,
    "null denominator list": _null_den,
    "null values": _no_values,
    "null blinds": _set("blinds", None),
    "null omega with a label factor": _set("omega", None),
    "null delta with a label factor": _set("delta", None),
    "n == 0": _set("n", 0),
    "usable_rows == n": _set("u", 8),
    "usable_rows > n": _set("u", 9),
    "n == 2^31": _set("n", 1 << 31),
    "field 1": _set("field", 1),
    "field 3": _set("field", 3),
    "field -1": _set("field", -1),
    "kind 3": _bad_kind,
    "kind 1 without a table": _no_table,
    "a job without factors": _no_factors,
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_return_zero_and_write_nothing(name):
    c = Call()
    REFUSALS[name](c)
    assert c.run() == 0
    assert c.untouched()


def test_refusals_whose_defect_is_the_output():
    c = Call()
    c.outs_arg = None
    assert c.run() == 0 and c.untouched()
    c = Call()
    c.outs[0] = None
    assert c.run() == 0
    for column in ("values", "table"):  # an output that aliases an input
        c = Call()
        before = getattr(c, column).raw
        c.outs[0] = ctypes.addressof(getattr(c, column))
        assert c.run() == 0
        assert getattr(c, column).raw == before
        c = Call()  # a partial overlap: the output starts inside the column
        c.outs[0] = ctypes.addressof(getattr(c, column)) + 32
        assert c.run() == 0


def test_python_wrapper_returns_none_on_a_refusal():
    from tachyon_amd import plonk
    col = R.encode(F, rand(43, 4))
    job = ([plonk.factor(col)], [plonk.factor(col)])
    assert plonk.grand_product_chains("bn254_fr", 4, 4, [[job]], None, None, []) is None
    with pytest.raises(ValueError):
        plonk.grand_product_chains("bn254_fr", 4, 2, [[job]], None, None, [])  # one blind is missing
    assert plonk.get_delta("bn254_fr") == fr(DELTA)
    Fb = R.field("bls12_381_fr")
    assert plonk.get_delta("bls12_381_fr") == Fb.to_bytes(R.get_delta(Fb))


def test_tile_accessors_are_positive():
    from tachyon_amd import plonk
    assert plonk.tile_rows() > 0 and plonk.walk_tiles() > 0
    assert plonk.tile_rows() % 64 == 0  # whole waves of rows
