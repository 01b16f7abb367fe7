"""The log-derivative lookup's m(X) and phi(X) on the GPU (tachyon_amd.log_lookup
over tachyon_mi355x_log_lookup_m_polys / _grand_sums) against
tests/log_lookup_ref.py, bytewise unless a test says otherwise.

The boundaries come from the library (tile_rows): usable rows around a tile's
end, zero denominators at a tile's first and last row, one size at which the
carry scan takes more than one step, and one size for each algorithm the
table's sort takes.
"""
import functools

import numpy as np
import pytest

import log_lookup_ref as R
from oracle import oracle as O
from oracle import pyref

pytestmark = pytest.mark.gpu

F = R.field("bn254_fr")
BETA = 0xBE7A


def tile():
    from tachyon_amd import log_lookup
    return log_lookup.tile_rows()


def rand(seed, count, field=F):
    return [pyref.rand_scalar(seed, i, field.p) for i in range(count)]


def pick(seed, count, modulus):
    return [pyref.rand_u64(seed, j) % modulus for j in range(count)]


@functools.lru_cache(maxsize=None)
def padded_table(seed, n, distinct, field=F):
    """n canonical values, `distinct` different ones: a table padded with duplicates, in no order."""
    base = rand(seed, distinct, field)
    return tuple(base[k] for k in pick(seed + 1, n, distinct))


def make_lookup(seed, n, u, K, distinct=37, miss_every=0, field=F):
    """(inputs, table) as canonical int lists: every input value occurs in
    the table's usable rows, but every miss_every-th row of input 0."""
    table = list(padded_table(seed, n, distinct, field))
    inputs = [[table[r] for r in pick(seed + 10 + k, n, u)] for k in range(K)]
    if miss_every:
        absent = [x for x in rand(seed + 5, 8, field) if x not in table][0]
        inputs[0] = [absent if j % miss_every == 0 else x for j, x in enumerate(inputs[0])]
    return inputs, table


def enc(cols, field=F):
    return [R.encode(field, c) for c in cols]


def check(n, u, lookups, beta=BETA, field=F, seed=1, m_override=None):
    """Both GPU calls on `lookups` (canonical int lists) against the
    reference; returns what the reference gave: (m ints, misses, phi ints, totals)."""
    from tachyon_amd import log_lookup as LL
    packed = [(enc(inputs, field), R.encode(field, table)) for inputs, table in lookups]
    want = [R.m_poly(field, n, u, inputs, table) for inputs, table in packed]
    got = LL.m_polys(field.name, n, u, packed)
    assert got is not None
    for k, (m_bytes, misses) in enumerate(want):
        assert got[0][k] == m_bytes, f"m of lookup {k} (n={n}, u={u})"
        assert got[1][k] == misses
    m = [w[0] for w in want] if m_override is None else [R.encode(field, x) for x in m_override]
    blinds = [rand(seed * 100 + k, n - u - 1, field) for k in range(len(lookups))]
    sums = [R.grand_sum(field, n, u, beta, inputs, table, m[k], blinds[k])
            for k, (inputs, table) in enumerate(packed)]
    got_phi = LL.grand_sums(field.name, n, u, field.to_bytes(beta), packed, m, [R.encode(field, b) for b in blinds])
    assert got_phi is not None
    for k, (phi, total) in enumerate(sums):
        assert got_phi[0][k] == phi, f"phi of lookup {k} (n={n}, u={u})"
        assert got_phi[0][k][32 * (u + 1):] == R.encode(field, blinds[k])  # the blinding rows, verbatim
        assert got_phi[0][k][32 * u:32 * (u + 1)] == bytes(32)
        assert got_phi[1][k] == total
    return ([R.decode(field, w[0]) for w in want], [w[1] for w in want],
            [R.decode(field, s[0]) for s in sums], [s[1] for s in sums])


# --- sizes -----------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
def test_sixteen_rows(K):
    m, misses, _, totals = check(16, 10, [make_lookup(20 + K, 16, 10, K, distinct=4)])
    assert misses == [0] and sum(m[0]) == 10 * K and totals == [F.to_bytes(0)]


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("spec", ["T-1", "T", "T+1", "n-2"])
def test_usable_rows_around_a_tile(spec, K):
    T = tile()
    n = 2 * T
    u = eval(spec, {"T": T, "n": n})
    m, misses, phi, totals = check(n, u, [make_lookup(30 + K, n, u, K, miss_every=97)], seed=K)
    assert misses == [len(range(0, u, 97))] and sum(m[0]) == K * u - misses[0]
    assert totals[0] != F.to_bytes(0)  # the misses unbalance it
    assert phi[0][0] == 0 and phi[0][u] == 0


def test_two_circuits_of_two_lookups_in_one_call():
    from tachyon_amd import log_lookup as LL
    T = tile()
    n, u = 2 * T, T + 5
    shapes = [(1, 5), (3, 64), (2, 1), (1, 300)]  # circuit 0's two lookups, then circuit 1's: (K, distinct values)
    lookups = [make_lookup(40 + 7 * k, n, u, K, distinct=d) for k, (K, d) in enumerate(shapes)]
    m, misses, _, totals = check(n, u, lookups)
    assert misses == [0] * 4 and totals == [F.to_bytes(0)] * 4
    # each lookup alone gives what it gave in the joint call
    for k in (1, 2):
        inputs, table = enc(lookups[k][0]), R.encode(F, lookups[k][1])
        alone = LL.m_polys("bn254_fr", n, u, [(inputs, table)])
        assert alone == ([R.encode(F, m[k])], [0])


def test_bls12_381_fr():
    Fb = R.field("bls12_381_fr")
    n = 2 * tile()
    u = n - 6
    top = Fb.p - 1  # the largest canonical value: every bit of the top limb's sorted range
    inputs, table = make_lookup(50, n, u, 2, field=Fb)
    table[3] = table[u - 1] = top
    inputs[1][0] = inputs[1][u - 1] = top
    check(n, u, [(inputs, table)], field=Fb)


# --- residency ---------------------------------------------------------------------
def test_host_and_device_inputs_and_out_tensors():
    import torch
    from tachyon_amd import log_lookup as LL
    n = 2 * tile()
    u = n - 3
    lookups = [make_lookup(60, n, u, 2), make_lookup(61, n, u, 1)]
    packed = [(enc(i), R.encode(F, t)) for i, t in lookups]
    want_m = [R.m_poly(F, n, u, i, t) for i, t in packed]
    blinds = [R.encode(F, rand(62 + k, n - u - 1)) for k in range(2)]
    want_phi = [R.grand_sum(F, n, u, BETA, i, t, want_m[k][0], R.decode(F, blinds[k]))
                for k, (i, t) in enumerate(packed)]

    def conv(f):
        return [([f(c) for c in i], f(t)) for i, t in packed]

    as_numpy = conv(lambda b: np.frombuffer(b, np.uint8).copy())
    as_cuda = conv(lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda())
    before = [c.clone() for i, t in as_cuda for c in i + [t]]
    for form in (as_numpy, as_cuda):
        got = LL.m_polys("bn254_fr", n, u, form)
        assert got == ([w[0] for w in want_m], [w[1] for w in want_m])
    out_m = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
    m, misses = LL.m_polys("bn254_fr", n, u, as_cuda, out=out_m)
    assert m[0] is out_m[0] and m[1] is out_m[1]
    assert [bytes(t.cpu().numpy()) for t in m] == [w[0] for w in want_m]
    # m stays on the device for the second call; blinds and beta come from the host
    out_phi = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
    phi, totals = LL.grand_sums("bn254_fr", n, u, F.to_bytes(BETA), as_cuda, out_m, blinds, out=out_phi)
    assert phi[0] is out_phi[0] and phi[1] is out_phi[1]
    assert [bytes(t.cpu().numpy()) for t in phi] == [w[0] for w in want_phi]
    assert totals == [w[1] for w in want_phi]
    # host columns with a device m, and host outputs
    phi, totals = LL.grand_sums("bn254_fr", n, u, F.to_bytes(BETA), as_numpy, out_m, blinds)
    assert phi == [w[0] for w in want_phi] and totals == [w[1] for w in want_phi]
    after = [c for i, t in as_cuda for c in i + [t]]
    assert all(torch.equal(a, b) for a, b in zip(before, after))  # inputs are never written

    # a device column at an address that is not 16-byte aligned is staged, not refused
    def shifted(b):
        t = torch.zeros(32 * n + 8, dtype=torch.uint8, device="cuda")
        t[8:] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
        assert t[8:].data_ptr() % 16 == 8
        return t[8:]
    unaligned = conv(shifted)
    out_u = [torch.zeros(32 * n + 8, dtype=torch.uint8, device="cuda")[8:] for _ in range(2)]
    m, _ = LL.m_polys("bn254_fr", n, u, unaligned, out=out_u)
    assert [bytes(t.cpu().numpy()) for t in m] == [w[0] for w in want_m]


# --- the sort's order ------------------------------------------------------------------
def test_values_that_differ_in_one_limb():
    """Tables whose values differ only in the top limb, only in the bottom
    limb, and pairs equal in three limbs, each value several times over: the
    counted rows follow the bisection over the exact canonical order."""
    n, u = 64, 61
    x = 0x1234_5678_9ABC_DEF0_0FED_CBA9_8765_4321_1111_2222_3333_4444_5555_6666_7777_8888 % (1 << 250)
    shifts = {"top": 192, "bottom": 0, "second": 64, "third": 128}
    lookups = []
    for k, (name, s) in enumerate(shifts.items()):
        # 7 values in descending table order, x with limb `s` replaced by 0..6 (top limb: only the low bits)
        base = x & ~(0xFFFF_FFFF_FFFF_FFFF << s)
        values = [base | ((6 - v) << s if s < 192 else (6 - v) << (s + 40)) for v in range(7)]
        table = [values[r] for r in pick(70 + k, n, 7)]
        # the same values, 2^32 apart within the limb: the limb's upper and lower half both matter
        table[5] = values[0] + (1 << (s + 32)) if s < 192 else values[0] + (1 << (s + 8))
        table[9] = values[0] + (1 << s)
        inputs = [[table[r] for r in pick(80 + k, n, u)]]
        lookups.append((inputs, table))
    m, misses, _, _ = check(n, u, lookups)
    assert misses == [0] * 4 and all(sum(x) == u for x in m)


def test_one_value_and_runs_of_duplicates():
    T = tile()
    n, u = 2 * T, 2 * T - 2
    # a table that is all one value: one row takes every count
    one = rand(90, 1)[0]
    m, _, _, _ = check(n, u, [([[one] * n, [one] * n], [one] * n)])
    assert sorted(m[0])[-1] == 2 * u and sum(m[0]) == 2 * u
    # runs whose lengths straddle the powers of two, the rows of a run scattered over the table
    lengths = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    values = rand(91, len(lengths) + 1)
    rows = [v for v, count in zip(values, lengths) for _ in range(count)]
    rows += [values[-1]] * (u - len(rows))
    order = np.random.default_rng(92).permutation(u)
    table = [rows[i] for i in order] + [values[-1]] * (n - u)
    inputs = [[values[k] for k in pick(93, n, len(values))], list(table)]
    m, misses, _, totals = check(n, u, [(inputs, table)])
    # each value occurs in the usable rows (the filler has hundreds of rows): no miss
    assert misses == [0] and totals == [F.to_bytes(0)]
    assert sum(1 for c in m[0] if c) == len(values)  # one counted row per value


def test_each_path_of_the_sort():
    """rocPRIM's radix_sort_pairs with the default configuration and 64-bit
    keys with 32-bit values takes one of three algorithms by the number of
    items (rocprim/device/device_radix_sort.hpp, radix_sort_impl): a single
    block sort up to 256 threads x 4 items = 1024, a block sort plus merge
    passes up to radix_sort_config<>::merge_sort_limit = 1024 * 1024 = 2^20,
    Onesweep above.  u = 1000 and u = 1500 take the first two against the
    reference (as do most tests here); Onesweep starts above 2^20, so this
    one case runs at u = 2^20 + 1, n = 2^21, without the Python reference:
    the table's values are distinct, so the counted row of an input taken
    from row r is r, and m is the histogram of the rows taken.  The values
    share their three upper limbs among few: a pass that was not stable would
    break the order the passes before it made, and the searches would miss."""
    from tachyon_amd import log_lookup as LL
    check(2048, 1000, [make_lookup(100, 2048, 1000, 1, distinct=700)])
    check(2048, 1500, [make_lookup(101, 2048, 1500, 1, distinct=900)])
    n, u = 1 << 21, (1 << 20) + 1
    rng = np.random.default_rng(102)
    limbs = np.zeros((n, 4), np.uint64)
    limbs[:, 0] = rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # distinct: odd multiplier
    limbs[:, 1] = rng.integers(0, 3, n)
    limbs[:, 2] = rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)
    limbs[:, 3] = rng.integers(0, 5, n).astype(np.uint64) << np.uint64(57)
    table = O.field_op("bn254_fr", "to_mont", limbs.tobytes())
    taken = rng.integers(0, u + u // 8, n)  # some from rows >= u: values that occur only there must miss
    inputs = np.frombuffer(table, np.uint8).reshape(n, 32)[taken].tobytes()
    got = LL.m_polys("bn254_fr", n, u, [([inputs], table)])
    assert got is not None
    counts = np.bincount(taken[:u][taken[:u] < u], minlength=n)
    small = np.frombuffer(R.encode(F, range(int(counts.max()) + 1)), np.uint8).reshape(-1, 32)
    assert got[0][0] == small[counts].tobytes()
    assert got[1] == [int((taken[:u] >= u).sum())]


# --- counting ------------------------------------------------------------------------------
def test_hot_counter_misses_and_values_past_the_usable_rows():
    T = tile()
    n, u = 2 * T, T + 300
    table = list(padded_table(110, n, 50))
    late = rand(111, 1)[0]  # occurs at rows >= u only
    table[u] = table[n - 1] = late
    absent = rand(112, 1)[0]
    hot = table[17]
    inputs = [[hot] * n,  # every add on one counter
              [absent] * n,  # nothing found: m unchanged, u misses
              [late if j % 2 else hot for j in range(n)]]  # half of them miss
    m, misses, _, totals = check(n, u, [(inputs, table)])
    assert misses == [u + u // 2]
    assert sum(m[0]) == u + (u + 1) // 2 and max(m[0]) == sum(m[0])
    assert totals[0] != F.to_bytes(0)


# --- the sums' edges ------------------------------------------------------------------------
def test_zero_denominators():
    T = tile()
    n, u = 2 * T, 2 * T - 1
    inputs, table = make_lookup(120, n, u, 2)
    zero = (-BETA) % F.p
    for j in (0, T - 1, T, u - 1):  # f + beta = 0 at a tile's first and last row
        inputs[0][j] = zero
    inputs[0][T + 1] = inputs[1][T + 1] = zero  # both inputs of one row
    table[7] = table[T + 1] = zero  # t + beta = 0 ...
    inputs[1][3] = inputs[1][4] = zero  # ... on rows that are counted: m != 0 there, the term is forced to 0
    m, _, phi, _ = check(n, u, [(inputs, table)])
    assert m[0][7] + m[0][T + 1] == 8
    L = R.log_derivative_terms(F, u, BETA, inputs, table, m[0])
    assert (phi[0][T + 2] - phi[0][T + 1]) % F.p == 0 == L[T + 1]  # a row that contributes nothing at all
    # an arbitrary m column (not the lookup's own) on the same rows
    check(n, u, [(inputs, table)], m_override=[rand(121, n)])


def test_a_carry_scan_of_more_than_one_step():
    """n = 2^19: 512 tiles per lookup, two steps of the 256-wide carry scan,
    two lookups in the call.  No Python reference at this size: with nonzero
    denominators the recurrence (phi[i+1] - phi[i]) (f + beta) (t + beta) =
    (t + beta) - m (f + beta), phi[0] = 0 and the returned total (which closes
    the recurrence at row u - 1) determine phi completely; they are checked
    elementwise with the oracle's C field operations."""
    from tachyon_amd import log_lookup as LL
    T = tile()
    n = 512 * T
    assert n // T > 256 and n <= 1 << 19
    u = n - 6
    fld = "bn254_fr"
    col = [O.gen_scalars(fld, 130 + k, n).tobytes() for k in range(6)]
    beta = F.to_bytes(BETA)
    blinds = [R.encode(F, rand(140 + k, n - u - 1)) for k in range(2)]
    lookups = [([col[0]], col[1]), ([col[3]], col[4])]
    m = [col[2], col[5]]
    phi, totals = LL.grand_sums(fld, n, u, beta, lookups, m, blinds)

    def op(name, a, b):
        return O.field_op(fld, name, a, b)

    for k, ((f,), t) in enumerate(lookups):
        z = phi[k]
        assert len(z) == 32 * n and z[:32] == bytes(32) and z[32 * u:32 * (u + 1)] == bytes(32)
        assert z[32 * (u + 1):] == blinds[k]
        fb, tb = op("add", f[:32 * u], beta * u), op("add", t[:32 * u], beta * u)
        for d in (fb, tb):  # every denominator is nonzero: the recurrence then leaves nothing out
            assert np.frombuffer(d, np.uint64).reshape(u, 4).any(axis=1).all()
        nxt = z[32:32 * u] + totals[k]  # phi[1..u-1], then the full sum
        lhs = op("mul", op("sub", nxt, z[:32 * u]), op("mul", fb, tb))
        assert lhs == op("sub", tb, op("mul", m[k][:32 * u], fb))
        top = np.frombuffer(z, np.uint64).reshape(n, 4)[:, 3]
        assert int(top.max()) <= F.p >> 192  # canonical output


# --- refusals ------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    import torch
    from tachyon_amd import log_lookup as LL
    from tachyon_amd._lib import lib
    n, u = 16, 10
    inputs, table = make_lookup(150, n, u, 2, distinct=4)
    f0, f1 = (torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda() for b in enc(inputs))
    t = torch.from_numpy(np.frombuffer(R.encode(F, table), np.uint8).copy()).cuda()
    m = torch.from_numpy(np.frombuffer(R.encode(F, rand(151, n)), np.uint8).copy()).cuda()
    out = torch.full((32 * n,), 0xAB, dtype=torch.uint8, device="cuda")
    blinds = R.encode(F, rand(152, n - u - 1))
    beta = F.to_bytes(BETA)
    good = [([f0, f1], t)]
    assert LL.m_polys("bn254_fr", n, u, good, out=[out.clone()]) is not None
    assert LL.grand_sums("bn254_fr", n, u, beta, good, [m], blinds, out=[out.clone()]) is not None

    def both(n_, u_, lookups, o, cols=()):
        """refused by both calls; cols: tensors of 32 n_ bytes where n_ differs"""
        bl = bytes(32 * max(0, n_ - u_ - 1))
        assert LL.m_polys("bn254_fr", n_, u_, lookups, out=[o]) is None
        assert LL.grand_sums("bn254_fr", n_, u_, beta, lookups, [cols[0] if cols else m], bl, out=[o]) is None

    def sized(rows):
        return torch.full((32 * rows,), 0xAB, dtype=torch.uint8, device="cuda")

    for rows, usable in ((12, 5), (1, 0), (24, 10)):  # no power of two; n < 2
        c = sized(rows)
        both(rows, usable, [([c], c.clone())], sized(rows), cols=[c.clone()])
    both(n, 0, good, out)
    both(n, n, good, out)
    both(n, n + 1, good, out)
    both(n, u, [([], t)], out)  # a lookup without inputs
    both(n, u, [(None, t)], out)
    both(n, u, [([f0, None], t)], out)
    both(n, u, [([f0], None)], out)
    both(n, u, good, None)  # a null output
    for alias in (f1, t):  # an output that is an input
        keep = alias.clone()
        both(n, u, good, alias)
        assert torch.equal(alias, keep)
    # the grand sums' own: beta, m, an output that is m, the blind count
    assert LL.grand_sums("bn254_fr", n, u, None, good, [m], blinds, out=[out]) is None
    assert LL.grand_sums("bn254_fr", n, u, beta, good, None, blinds, out=[out]) is None
    assert LL.grand_sums("bn254_fr", n, u, beta, good, [None], blinds, out=[out]) is None
    keep = m.clone()
    assert LL.grand_sums("bn254_fr", n, u, beta, good, [m], blinds, out=[m]) is None
    assert torch.equal(m, keep)
    assert LL.grand_sums("bn254_fr", n, u, beta, good, [m], blinds[32:], out=[out]) is None
    assert LL.grand_sums("bn254_fr", n, u, beta, good, [m], blinds + bytes(32), out=[out]) is None
    # the field, through the entry points themselves: 1 and 3 are the curves' base fields elsewhere
    cols = LL._Columns(n)
    arr = LL._descriptors(cols, good)
    outs, _ = LL._outputs(cols, [out], 1, n)
    mptr = (LL.ctypes.c_void_p * 1)(m.data_ptr())
    for field in (1, 3, -1):
        assert lib().tachyon_mi355x_log_lookup_m_polys(field, n, u, arr, 1, outs, None) == 0
        assert lib().tachyon_mi355x_log_lookup_grand_sums(field, n, u, beta, arr, mptr, 1, blinds, outs, None) == 0
    # a null blinds pointer where there are blind rows
    assert lib().tachyon_mi355x_log_lookup_grand_sums(0, n, u, beta, arr, mptr, 1, None, outs, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    # nothing to do is no refusal
    assert LL.m_polys("bn254_fr", n, u, []) == ([], [])
    assert lib().tachyon_mi355x_log_lookup_work_bytes(1 << 16, 2, 3) > 3 * 4 * 32 << 16


# --- into the existing path ----------------------------------------------------------------------
def test_device_m_and_phi_commit():
    import torch
    from tachyon_amd import log_lookup as LL
    from tachyon_amd.kzg import KZG
    n, u = 16, 10
    inputs, table = make_lookup(160, n, u, 2, distinct=4)
    packed = [(enc(inputs), R.encode(F, table))]
    want_m, _ = R.m_poly(F, n, u, *packed[0])
    blinds = rand(161, n - u - 1)
    want_phi, _ = R.grand_sum(F, n, u, BETA, packed[0][0], packed[0][1], want_m, blinds)
    as_cuda = [([torch.from_numpy(np.frombuffer(c, np.uint8).copy()).cuda() for c in packed[0][0]],
                torch.from_numpy(np.frombuffer(packed[0][1], np.uint8).copy()).cuda())]
    m_dev = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda")]
    phi_dev = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda")]
    assert LL.m_polys("bn254_fr", n, u, as_cuda, out=m_dev) is not None
    assert LL.grand_sums("bn254_fr", n, u, F.to_bytes(BETA), as_cuda, m_dev, [R.encode(F, blinds)],
                         out=phi_dev) is not None
    kzg = KZG("bn254_g1")
    kzg.unsafe_setup(n, F.to_bytes(0x7A0))
    assert kzg.commit_lagrange(m_dev[0]) == kzg.commit_lagrange(want_m)
    assert kzg.commit_lagrange(phi_dev[0]) == kzg.commit_lagrange(want_phi)
    kzg.close()
    ms = LL.last_timings()
    assert set(ms) == set(LL.PHASES) and all(v >= 0 for v in ms.values())
