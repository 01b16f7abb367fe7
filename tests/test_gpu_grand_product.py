"""Halo2 grand products on the GPU (tachyon_amd.plonk over
tachyon_mi355x_grand_product_chains) against tests/grand_product_ref.py,
bytewise unless a test says otherwise.

The boundaries come from the library (tile_rows, walk_tiles): rows around a
tile's end, usable rows around it, chains that continue across jobs and
tiles, zero denominators at a tile's first row, and one size at which the
carry walk takes more than one step.
"""
import functools

import numpy as np
import pytest

import grand_product_ref as R
import halo2_golden as H
from oracle import oracle as O
from oracle import pyref

pytestmark = pytest.mark.gpu

F = H.FR
DELTA = R.get_delta(F)
OMEGA = F.root_of_unity(1 << 24)  # labels need only some omega; its powers are distinct over every size here
PERM_CASES = [c for c in H.circuits() if c.get("permutations_columns")]
PERM_IDS = [H.case_id(c) for c in PERM_CASES]


def fr(x, field=F):
    return field.to_bytes(x)


def rand(seed, count, field=F):
    return [pyref.rand_scalar(seed, i, field.p) for i in range(count)]


@functools.lru_cache(maxsize=None)
def column(seed, n, field_name="bn254_fr"):
    return O.gen_scalars(field_name, seed, n).tobytes()


def tile():
    from tachyon_amd import plonk
    return plonk.tile_rows()


def check(n, u, chains, omega=OMEGA, delta=DELTA, seed=1, field=F):
    """One GPU call against the reference; returns the decoded reference rows and last values."""
    from tachyon_amd import plonk
    jobs = sum(len(c) for c in chains)
    blinds = [rand(seed * 100 + k, n - u - 1, field) for k in range(jobs)]
    want_z, want_last = R.grand_product_chains(field, n, u, chains, omega, delta, blinds)
    got = plonk.grand_product_chains(field.name, n, u, chains, fr(omega, field), fr(delta, field),
                                     [R.encode(field, b) for b in blinds])
    assert got is not None
    for k in range(jobs):
        assert got[0][k] == want_z[k], f"job {k} (n={n}, u={u})"
    assert got[1] == want_last
    return want_z, want_last, blinds


def simple_job(n, seed):
    return ([R.factor(column(seed, n), c=fr(3))], [R.factor(column(seed + 1, n), c=fr(5))])


def mixed_job(n, seed, field=F):
    """4 + 4 factors over the three kinds; columns shared between the sides."""
    c = [column(seed + k, n, field.name) for k in range(8)]
    beta, gamma, beta2 = fr(0xBE7A, field), fr(0x6A33A, field), fr(0x1234567, field)
    num = [R.factor(c[0], c=gamma), R.factor(c[1], m=beta, table=c[2], c=gamma),
           R.factor(c[3], m=beta, label=0, c=gamma), R.factor(c[4], m=beta2, label=5)]
    den = [R.factor(c[0], m=beta, table=c[5], c=gamma), R.factor(c[6], c=beta2),
           R.factor(c[7], m=beta, label=2, c=gamma), R.factor(c[1], m=beta2, table=c[4])]
    return num, den


# --- golden circuits -------------------------------------------------------------
def perm_setup(c):
    n, omega = c["n"], int(c["omega"], 16)
    sig = [[int(h, 16) for h in col] for col in c["permutations_columns"]]
    return n, omega, sig, H.indicator_polys(c)["u"]


@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("c", PERM_CASES, ids=PERM_IDS)
def test_golden_circuit_permutations(c, L):
    from tachyon_amd import plonk
    n, omega, sig, u = perm_setup(c)
    sigmas = [R.encode(F, col) for col in sig]
    beta, gamma = fr(0xBE7A), fr(0x6A33A)
    # random witnesses, two circuits in one call: bytes and last values equal the reference's
    values = [[column(300 + 10 * k + i, n) for i in range(len(sig))] for k in range(2)]
    chains = R.permutation_chains(values, sigmas, beta, gamma, L + 2)
    jobs = sum(len(ch) for ch in chains)
    blinds = [rand(60 + k, n - u - 1) for k in range(jobs)]
    want_z, want_last = R.grand_product_chains(F, n, u, chains, omega, DELTA, blinds)
    got = plonk.permutation_grand_products(values, sigmas, beta, gamma, L + 2, n, u, fr(omega),
                                           blinds=[R.encode(F, b) for b in blinds])
    assert [z for circuit in got[0] for z in circuit] == want_z
    assert [len(circuit) for circuit in got[0]] == [len(ch) for ch in chains]
    assert got[1] == want_last
    # a witness constant on every cycle closes the product
    cells = R.decode_sigmas(F, sig, omega, DELTA)
    w = [R.encode(F, col) for col in R.cycle_constant_witness(F, cells, 900 + L)]
    _, last = plonk.permutation_grand_products([w], sigmas, beta, gamma, L + 2, n, u, fr(omega),
                                               blinds=[R.encode(F, b) for b in blinds[:len(chains[0])]])
    assert last == [fr(1)]


# --- row boundaries ----------------------------------------------------------------
ROWS = ["1", "2", "63", "64", "65", "T-1", "T", "T+1", "2T+3"]


def rows_of(spec):
    return eval(spec.replace("2T", "2*T"), {"T": tile()})


@pytest.mark.parametrize("spec", ROWS)
def test_row_boundaries(spec):
    T = tile()
    n = rows_of(spec)
    us = sorted({u for u in (0, 1, T - 1, T, T + 1, n - 1) if u < n})
    assert us
    for u in us:
        for job in (simple_job(n, 10), mixed_job(n, 20)):
            want_z, want_last, blinds = check(n, u, [[job]], seed=u + 1)
            if u == 0:  # z = [1, blinds...]
                assert want_z[0] == fr(1) + R.encode(F, blinds[0]) and want_last == [fr(1)]
                assert len(blinds[0]) == n - 1  # none at n = 1


# --- chains ------------------------------------------------------------------------
def five_columns(n, seed):
    values = [column(seed + i, n) for i in range(5)]
    sigmas = [column(seed + 50 + i, n) for i in range(5)]
    return values, sigmas


def test_chain_over_column_chunks_and_two_chains_in_one_call():
    from tachyon_amd import plonk
    T = tile()
    n, u = 2 * T + 3, 2 * T
    beta, gamma = fr(0xBE7A), fr(0x6A33A)
    va, sigmas = five_columns(n, 400)
    vb, _ = five_columns(n, 500)
    chains = R.permutation_chains([va, vb], sigmas, beta, gamma, 4)
    assert [len(ch) for ch in chains] == [3, 3]
    assert [len(num) for num, _ in chains[0]] == [2, 2, 1]
    want_z, want_last, blinds = check(n, u, chains)
    rows = [R.decode(F, z) for z in want_z]
    for k in (1, 2, 4, 5):  # the chain rule on what the GPU call returned too
        assert rows[k][0] == rows[k - 1][u]
    # each chain alone gives what it gave in the joint call
    for c in range(2):
        got = plonk.grand_product_chains("bn254_fr", n, u, [chains[c]], fr(OMEGA), fr(DELTA),
                                         [R.encode(F, b) for b in blinds[3 * c:3 * c + 3]])
        assert got[0] == want_z[3 * c:3 * c + 3] and got[1] == [want_last[c]]


@pytest.mark.parametrize("where", ["row 0", "first row of a tile", "row u-1", "three in a row"])
def test_zero_denominator_in_the_middle_job(where):
    T = tile()
    n, u = 2 * T + 3, 2 * T
    at = {"row 0": [0], "first row of a tile": [T], "row u-1": [u - 1], "three in a row": [T - 1, T, T + 1]}[where]
    beta, gamma = 0xBE7A, 0x6A33A
    values, sigmas = five_columns(n, 600)
    # column 2 (the middle job's first): v = -beta sigma - gamma on the chosen rows
    v2, s2 = R.decode(F, values[2]), R.decode(F, sigmas[2])
    for j in at:
        v2[j] = (-beta * s2[j] - gamma) % F.p
    values = values[:2] + [R.encode(F, v2)] + values[3:]
    chains = R.permutation_chains([values], sigmas, fr(beta), fr(gamma), 4)
    want_z, want_last, _ = check(n, u, chains)
    r0, r1, r2 = (R.decode(F, z) for z in want_z)
    assert all(x != 0 for x in r0[:u + 1])
    assert all(x != 0 for x in r1[:at[0] + 1])
    assert r1[at[0] + 1:u + 1] == [0] * (u - at[0])  # everything after is 0
    assert r2[:u + 1] == [0] * (u + 1) and want_last == [fr(0)]  # and the next job starts from 0


# --- wrappers, residency, BLS12-381 ---------------------------------------------------
def test_lookup_and_shuffle_wrappers():
    from tachyon_amd import plonk
    n = tile() + 1
    u = n - 4
    A, S, Ap, Sp = (column(700 + k, n) for k in range(4))
    beta, gamma = fr(17), fr(19)
    blinds = rand(71, n - u - 1)
    want_z, want_last = R.grand_product_chains(F, n, u, [[R.lookup_job(A, S, Ap, Sp, beta, gamma)]], 1, 1, [blinds])
    assert plonk.lookup_grand_product(A, S, Ap, Sp, beta, gamma, n, u, blinds=R.encode(F, blinds)) == \
        (want_z[0], want_last[0])
    want_z, want_last = R.grand_product_chains(F, n, u, [[R.shuffle_job(A, S, gamma)]], 1, 1, [blinds])
    assert plonk.shuffle_grand_product(A, S, gamma, n, u, blinds=[R.encode(F, blinds)]) == (want_z[0], want_last[0])


def test_residency():
    import torch
    from tachyon_amd import plonk
    n = tile() + 1
    u = n - 3
    num, den = mixed_job(n, 800)
    chains = [[(num, den), simple_job(n, 810)]]
    want_z, want_last, blinds = check(n, u, chains)
    bl = [R.encode(F, b) for b in blinds]
    args = ("bn254_fr", n, u)

    def convert(chains, conv):
        seen = {}

        def one(x):
            if x is None:
                return None
            if id(x) not in seen:
                seen[id(x)] = conv(x)
            return seen[id(x)]
        return [[tuple([dict(f, values=one(f["values"]), table=one(f["table"])) for f in side] for side in job)
                 for job in chain] for chain in chains], seen

    as_numpy, _ = convert(chains, lambda b: np.frombuffer(b, np.uint8).copy())
    assert plonk.grand_product_chains(*args, as_numpy, fr(OMEGA), fr(DELTA), bl) == (want_z, want_last)

    as_cuda, tensors = convert(chains, lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda())
    before = [t.clone() for t in tensors.values()]
    assert plonk.grand_product_chains(*args, as_cuda, fr(OMEGA), fr(DELTA), bl) == (want_z, want_last)
    out = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
    z, last = plonk.grand_product_chains(*args, as_cuda, fr(OMEGA), fr(DELTA), bl, out=out)
    assert [bytes(t.cpu().numpy()) for t in z] == want_z and last == want_last
    assert z[0] is out[0] and z[1] is out[1]
    assert all(torch.equal(a, b) for a, b in zip(before, tensors.values()))  # inputs are never written

    # a device column at an address that is not 16-byte aligned is staged, not refused
    def shifted(b):
        t = torch.zeros(32 * n + 8, dtype=torch.uint8, device="cuda")
        t[8:] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
        view = t[8:]
        assert view.data_ptr() % 16 == 8
        return view
    unaligned, _ = convert(chains, shifted)
    out_u = [torch.zeros(32 * n + 8, dtype=torch.uint8, device="cuda")[8:] for _ in range(2)]
    z, last = plonk.grand_product_chains(*args, unaligned, fr(OMEGA), fr(DELTA), bl, out=out_u)
    assert [bytes(t.cpu().numpy()) for t in z] == want_z and last == want_last


def test_bls12_381_fr():
    Fb = R.field("bls12_381_fr")
    n = tile() + 1
    chains = [[mixed_job(n, 900, Fb), mixed_job(n, 910, Fb)]]
    check(n, n - 5, chains, omega=Fb.root_of_unity(1 << 20), delta=R.get_delta(Fb), field=Fb)


# --- past the carry walk's first step -------------------------------------------------
def test_recurrence_past_the_walks_first_step():
    """n = min(2^22, the smallest power of two with n / tile_rows > walk_tiles):
    one chain of two jobs whose tile products take more than one step of the
    carry walk per job.  No Python reference at this size: with nonzero
    denominators the recurrence z[j+1] den(j) = z[j] num(j), z[0] and the
    blinds determine Z completely, and they are checked elementwise with the
    oracle's C field operations.  (Were walk_tiles * tile_rows >= 2^22 the case
    would run at 2^22 and not reach the walk's second step; with 1024-row
    tiles and 256 products per step it runs at 2^19 and does.)"""
    from tachyon_amd import plonk
    T, W = plonk.tile_rows(), plonk.walk_tiles()
    n = 1
    while n // T <= W and n < 1 << 22:
        n *= 2
    u = n - 6
    fld = "bn254_fr"
    c = [column(1000 + k, n) for k in range(5)]
    beta, gamma = fr(0xBE7A), fr(0x6A33A)

    def rep(x):
        return x * n

    def mul(a, b):
        return O.field_op(fld, "mul", a, b)

    def add(a, b):
        return O.field_op(fld, "add", a, b)

    # labels delta^1 omega^j for j < n (past the 65536-row table boundary)
    lab, x = [], DELTA
    for _ in range(n):
        lab.append(x)
        x = x * OMEGA % F.p
    lab = b"".join((v * F.R % F.p).to_bytes(32, "little") for v in lab)
    jobs = [([R.factor(c[0], c=gamma), R.factor(c[1], m=beta, label=1, c=gamma)],
             [R.factor(c[0], m=beta, table=c[2], c=gamma)]),
            ([R.factor(c[3], c=beta)], [R.factor(c[4], c=gamma), R.factor(c[2], m=beta, table=c[3])])]
    nums = [mul(add(c[0], rep(gamma)), add(add(c[1], mul(lab, rep(beta))), rep(gamma))), add(c[3], rep(beta))]
    dens = [add(add(c[0], mul(c[2], rep(beta))), rep(gamma)),
            mul(add(c[4], rep(gamma)), add(c[2], mul(c[3], rep(beta))))]
    for d in dens:  # every denominator is nonzero: the recurrence then leaves nothing out
        assert np.frombuffer(d, np.uint64).reshape(n, 4).any(axis=1).all()
    blinds = [R.encode(F, rand(80 + k, n - u - 1)) for k in range(2)]
    z, last = plonk.grand_product_chains(fld, n, u, [jobs], fr(OMEGA), fr(DELTA), blinds)
    assert z[0][:32] == fr(1)
    assert z[1][:32] == z[0][32 * u:32 * (u + 1)]
    assert last == [z[1][32 * u:32 * (u + 1)]]
    for k in range(2):
        assert len(z[k]) == 32 * n
        assert mul(z[k][32:32 * (u + 1)], dens[k][:32 * u]) == mul(z[k][:32 * u], nums[k][:32 * u])
        assert z[k][32 * (u + 1):] == blinds[k]
        # canonical output: every element is below the modulus
        top = np.frombuffer(z[k], np.uint64).reshape(n, 4)[:, 3]
        assert int(top.max()) <= F.p >> 192


# --- into the existing path -----------------------------------------------------------
def test_device_z_commits_and_transforms():
    import torch
    from tachyon_amd import plonk
    from tachyon_amd.kzg import KZG
    from tachyon_amd.ntt import Radix2EvaluationDomain, ScopedSubgroupGeneratorOverrider
    c = PERM_CASES[0]
    n, omega, sig, u = perm_setup(c)
    sigmas = [R.encode(F, col) for col in sig]
    values = [[column(1100 + i, n) for i in range(len(sig))]]
    beta, gamma = fr(0xBE7A), fr(0x6A33A)
    chains = R.permutation_chains(values, sigmas, beta, gamma, 4)
    blinds = [rand(90 + k, n - u - 1) for k in range(len(chains[0]))]
    want_z, _ = R.grand_product_chains(F, n, u, chains, omega, DELTA, blinds)
    out = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in chains[0]]
    got = plonk.permutation_grand_products(values, sigmas, beta, gamma, 4, n, u, fr(omega),
                                           blinds=[R.encode(F, b) for b in blinds], out=out)
    assert got is not None
    kzg = KZG("bn254_g1")
    with ScopedSubgroupGeneratorOverrider():
        kzg.unsafe_setup(16, fr(H.TAU))
        dom = Radix2EvaluationDomain(n)
    for z_dev, z_ref in zip(out, want_z):
        assert bytes(z_dev.cpu().numpy()) == z_ref
        assert kzg.commit_lagrange(z_dev) == kzg.commit_lagrange(z_ref)
        work = z_dev.clone()
        dom.transform_device(work.data_ptr(), inverse=True)
        torch.cuda.synchronize()
        assert bytes(work.cpu().numpy()) == dom.ifft(z_ref).ljust(32 * n, b"\0")
        dom.transform_device(work.data_ptr(), inverse=False)
        torch.cuda.synchronize()
        assert torch.equal(work, z_dev)
    dom.close()
    kzg.close()
