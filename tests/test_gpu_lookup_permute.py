"""The Halo2 lookup's permuted columns A' and S' on the GPU
(tachyon_amd.lookup_permute over tachyon_mi355x_lookup_permute_pairs) against
tests/lookup_permute_ref.py, bytewise.

The boundaries come from the code: kLpBlock (plonk/lookup_permute.h) is both
the new kernels' workgroup and the scan's tile, the carry scan takes kLpBlock
tile counts per step, and rocPRIM's radix sort changes its algorithm above
1024 and above 2^20 items (see test_the_onesweep_sort).
"""
import functools
import os
import re

import numpy as np
import pytest

import lookup_permute_ref as R
from oracle import oracle as O
from oracle import pyref

pytestmark = pytest.mark.gpu

F = R.field("bn254_fr")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block():
    """Threads of a workgroup of the new kernels = rows of a scan tile."""
    text = open(os.path.join(ROOT, "tachyon_amd", "csrc", "plonk", "lookup_permute.h")).read()
    return int(re.search(r"constexpr unsigned kLpBlock = (\d+);", text).group(1))


@functools.lru_cache(maxsize=None)
def pool(seed, count, field=F):
    """`count` distinct canonical values in ascending order."""
    values = sorted(set(pyref.rand_scalar(seed, i, field.p) for i in range(count + 8)))
    assert len(values) >= count
    return tuple(values[:count])


def pick(seed, count, modulus):
    return [pyref.rand_u64(seed, j) % modulus for j in range(count)]


def shuffled(seed, xs):
    order = np.random.default_rng(seed).permutation(len(xs))
    return [xs[i] for i in order]


def absent(seed, n, u, table, field=F):
    """n - u values that occur nowhere in the table: the rows past the usable ones."""
    have = set(table)
    base = (1 << 200) + (seed << 64)
    out = [x for x in range(base, base + 2 * (n - u) + 8) if x not in have]
    return out[:n - u]


def make_pair(seed, n, u, distinct, field=F):
    """(A, S) as canonical ints: a table of `distinct` values padded with
    duplicates in no order, inputs picked from its usable rows; the rows >= u
    of both hold values the table's usable rows do not have."""
    values = pool(seed, distinct, field)
    S = [values[k] for k in pick(seed + 1, u, distinct)]
    A = [S[r] for r in pick(seed + 2, u, u)]
    return A + absent(seed + 3, n, u, S, field), S + absent(seed + 4, n, u, S, field)


def as_cuda(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()


def check(n, u, pairs, field=F, seed=1, convert=None, out=False):
    """One GPU call on `pairs` (canonical int lists) against the reference.
    A pair the reference refuses must report its misses and still receive its
    blind rows.  Returns per pair (A' ints, S' ints) or None, and the misses."""
    import torch
    from tachyon_amd import lookup_permute as LP
    packed = [(R.encode(field, A), R.encode(field, S)) for A, S in pairs]
    blinds = [O.gen_scalars(field.name, seed * 1000 + k, 2 * (n - u)).tobytes() for k in range(len(pairs))]
    want = [R.permute_rows(u, A, S) for A, S in pairs]
    given = packed if convert is None else [(convert(A), convert(S)) for A, S in packed]
    outs = None
    if out:
        outs = [tuple(torch.full((32 * n,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)) for _ in pairs]
    got = LP.permute_pairs(field.name, n, u, given, blinds, out=outs)
    assert got is not None
    a_perm, s_perm, misses = got
    if out:
        assert all(a_perm[k] is outs[k][0] and s_perm[k] is outs[k][1] for k in range(len(pairs)))
        a_perm, s_perm = ([bytes(t.cpu().numpy()) for t in col] for col in (a_perm, s_perm))
    result = []
    for k, (A, S) in enumerate(pairs):
        assert misses[k] == R.misses(u, A, S), f"misses of lookup {k} (n={n}, u={u})"
        assert len(a_perm[k]) == len(s_perm[k]) == 32 * n
        # the blind rows, verbatim: n - u for A', then n - u for S'
        assert a_perm[k][32 * u:] == blinds[k][:32 * (n - u)]
        assert s_perm[k][32 * u:] == blinds[k][32 * (n - u):]
        if want[k] is None:
            assert misses[k] > 0
            result.append(None)
            continue
        assert misses[k] == 0
        assert a_perm[k][:32 * u] == R.encode(field, want[k][0]), f"A' of lookup {k} (n={n}, u={u})"
        assert s_perm[k][:32 * u] == R.encode(field, want[k][1]), f"S' of lookup {k} (n={n}, u={u})"
        result.append(want[k])
    return result, misses


def repeated_rows(a_perm):
    return sum(1 for i in range(1, len(a_perm)) if a_perm[i] == a_perm[i - 1])


# --- sizes -----------------------------------------------------------------------
def hand_worked():
    """n = 16, u = 10: the two hand-worked cases in rows 0..3, six rows of
    larger values that each map to themselves behind them."""
    tail0, tail1 = [25, 21, 24, 20, 23, 22], [33, 30, 35, 31, 34, 32]
    pairs = [([1, 2, 1, 5] + tail0 + [90] * 6, [1, 2, 4, 5] + sorted(tail0) + [91] * 6),
             ([1, 1, 1, 2] + tail1 + [92] * 6, [1, 1, 2, 4] + tail1[::-1] + [93] * 6)]
    want = [([1, 1, 2, 5] + sorted(tail0), [1, 4, 2, 5] + sorted(tail0)),
            ([1, 1, 1, 2] + sorted(tail1), [1, 4, 1, 2] + sorted(tail1))]
    return pairs, want


def test_sixteen_rows_host_columns():
    pairs, want = hand_worked()
    got, misses = check(16, 10, pairs)
    assert [tuple(g) for g in got] == want and misses == [0, 0]
    # interleaved with the rest rather than in front of it: the same rows come out
    mixed = [(A[4:10] + A[:4] + A[10:], S[4:10] + S[:4] + S[10:]) for A, S in pairs]
    got, _ = check(16, 10, mixed, seed=2)
    assert [tuple(g) for g in got] == want


def test_sixteen_rows_cuda_tensors_and_out():
    pairs, want = hand_worked()
    got, misses = check(16, 10, pairs, convert=as_cuda, out=True)
    assert [tuple(g) for g in got] == want and misses == [0, 0]
    # device columns, host results; host (numpy) columns, device results
    check(16, 10, pairs, convert=as_cuda)
    check(16, 10, pairs, convert=lambda b: np.frombuffer(b, np.uint8).copy(), out=True)


def straddling(seed, n, u, at):
    """A pair whose sorted inputs hold one value from row at - 3 to row at + 2
    (or to the last row): the first-row flag of row `at` needs the last key of
    the workgroup before it, and the run's ranks cross the scan tile's end."""
    values = pool(seed, u)
    lo = max(0, at - 3)
    hi = min(u, at + 3)
    ranks = list(range(lo)) + [lo] * (hi - lo) + list(range(hi, u))
    S = shuffled(seed + 1, list(values))
    A = shuffled(seed + 2, [values[r] for r in ranks])
    return A + absent(seed + 3, n, u, S), S + absent(seed + 4, n, u, S)


@pytest.mark.parametrize("spec", ["B-1", "B", "B+1", "2*B", "2*B+1", "3*B-1"])
def test_usable_rows_around_a_workgroup_and_scan_tile(spec):
    B = block()
    u = eval(spec, {"B": B})
    n = 1 << u.bit_length()  # the smallest power of two above u
    pairs = [straddling(10, n, u, B), make_pair(11, n, u, distinct=u // 3),
             straddling(12, n, u, 2 * B) if u > 2 * B else make_pair(12, n, u, distinct=5)]
    got, misses = check(n, u, pairs)
    assert misses == [0, 0, 0]
    a_perm = got[0][0]
    if u > B:
        assert a_perm[B] == a_perm[B - 1] and a_perm[B] != a_perm[B - 4]  # the run does straddle row B
    assert repeated_rows(a_perm) == min(u, B + 3) - max(0, B - 3) - 1


def test_a_carry_scan_of_more_than_one_step():
    """More than kLpBlock tiles per lookup: the carry kernel walks twice."""
    B = block()
    u = B * B + B + 7
    n = 1 << u.bit_length()
    assert n <= 1 << 17
    got, misses = check(n, u, [make_pair(20, n, u, distinct=u // 2)])
    assert misses == [0] and repeated_rows(got[0][0]) > B * B // 2  # ranks beyond one step's tiles


@pytest.mark.parametrize("u", [1023, 1024, 1025])
def test_the_one_block_sort_limit(u):
    """rocPRIM's radix_sort_pairs sorts up to 256 threads x 4 items = 1024 in
    one block and merges block sorts above that (see test_the_onesweep_sort)."""
    n = 1 << u.bit_length()
    _, misses = check(n, u, [make_pair(30, n, u, distinct=700), make_pair(31, n, u, distinct=u)])
    assert misses == [0, 0]


def test_the_onesweep_sort():
    """rocPRIM's radix_sort_pairs with the default configuration and 64-bit
    keys with 32-bit values takes a single block sort up to 1024 items, block
    sorts plus merge passes up to radix_sort_config<>::merge_sort_limit =
    2^20, Onesweep above (rocprim/device/device_radix_sort.hpp,
    radix_sort_impl).  One case at u = 2^20 + 1, n = 2^21, one lookup, without
    the Python walk: the table's usable rows are distinct values whose rank is
    known by construction, so the closed form is a few numpy lines over the
    ranks.  The values share their three upper limbs among few: a pass that
    was not stable would break the order the passes before it made."""
    from tachyon_amd import lookup_permute as LP
    n, u = 1 << 21, (1 << 20) + 1
    rng = np.random.default_rng(40)
    k = np.arange(n, dtype=np.uint64)  # value k: ascending in k, limb 3 first
    limbs = np.zeros((n, 4), np.uint64)
    limbs[:, 0] = (k & np.uint64(0x7FFF)) * np.uint64(0x0001_0000_0000_0001)
    limbs[:, 1] = (k >> np.uint64(15)) & np.uint64(3)
    limbs[:, 2] = ((k >> np.uint64(17)) & np.uint64(1)) << np.uint64(63)
    limbs[:, 3] = (k >> np.uint64(18)) << np.uint64(57)
    mont = np.frombuffer(O.field_op("bn254_fr", "to_mont", limbs.tobytes()), np.uint8).reshape(n, 32)
    s_rank = np.concatenate([rng.permutation(u), np.arange(u, n)])  # row -> rank of its value; past u: other values
    taken = np.concatenate([rng.integers(0, u, u), rng.integers(u, n, n - u)])  # row of S an input row copies
    a_rank = s_rank[taken]
    blinds = O.gen_scalars("bn254_fr", 41, 2 * (n - u)).tobytes()
    got = LP.permute_pairs("bn254_fr", n, u, [(mont[a_rank].tobytes(), mont[s_rank].tobytes())], blinds)
    assert got is not None and got[2] == [0]
    a_sorted = np.sort(a_rank[:u])
    first = np.concatenate([[True], a_sorted[1:] != a_sorted[:-1]])
    leftover = np.setdiff1d(np.arange(u), a_sorted)  # ascending; the table has every rank < u once
    R_ = int((~first).sum())
    assert len(leftover) == R_ and R_ > u // 4
    s_want = a_sorted.copy()
    s_want[~first] = leftover[R_ - 1 - np.arange(R_)]
    assert got[0][0] == mont[a_sorted].tobytes() + blinds[:32 * (n - u)]
    assert got[1][0] == mont[s_want].tobytes() + blinds[32 * (n - u):]


# --- contents ------------------------------------------------------------------------
N_MID, U_MID = 4096, 4001


def mid(A, S, seed=50):
    return A + absent(seed, N_MID, U_MID, S), S + absent(seed + 1, N_MID, U_MID, S)


def test_degenerate_contents():
    u = U_MID
    values = pool(51, u)
    one = values[1234]
    runs = [v for v, length in zip(values, [1, 2, 3, 255, 256, 257, 511, 513, 1000]) for _ in range(length)]
    runs += list(values[100:100 + u - len(runs)])
    pairs = [
        mid([one] * u, shuffled(52, list(values))),  # all inputs one value: R = u - 1
        mid(shuffled(53, list(values)), shuffled(54, list(values))),  # a permutation of a duplicate-free table: R = 0
        mid([one] * u, [one] * u),  # table and inputs all one value
        # long runs of duplicates in the table, the inputs use the values of some
        mid([runs[r] for r in pick(55, u, 600)], shuffled(56, runs)),
    ]
    got, misses = check(N_MID, u, pairs)
    assert misses == [0] * 4
    assert [repeated_rows(g[0]) for g in got[:3]] == [u - 1, 0, u - 1]
    assert got[0][1][0] == one and sorted(got[0][1]) == list(values)
    assert got[1][0] == got[1][1] == list(values)
    assert got[2][1] == [one] * u


def test_values_that_differ_in_one_limb_and_the_extremes():
    """Values equal in three limbs that differ only in limb 0, only in limb 3,
    only across the 16-byte halves of the search's compare, and 0 and p - 1."""
    u = U_MID
    x = 0x1234_5678_9ABC_DEF0_0FED_CBA9_8765_4321_1111_2222_3333_4444_5555_6666_7777_8888 % (1 << 250)
    groups = {
        "limb 0": [x ^ (v << 0) for v in (1, 2, 3, 1 << 31, 1 << 32, 1 << 63)],
        "limb 3": [x ^ (v << 192) for v in (1, 2, 3, 1 << 31, 1 << 32, 1 << 57)],
        "halves": [x ^ (1 << 127), x ^ (1 << 128), x ^ (3 << 127), x, x ^ (1 << 64), x ^ (1 << 191)],
        "extremes": [0, 1, F.p - 1, F.p - 2, (1 << 128) - 1, 1 << 128],
    }
    pairs = []
    for k, values in enumerate(groups.values()):
        assert len(set(values)) == 6 and all(0 <= v < F.p for v in values)
        S = [values[r] for r in pick(60 + k, u, 6)]
        A = [values[r] for r in pick(70 + k, u, 5 if k % 2 else 6)]  # one value of the table unused in two groups
        assert set(A) <= set(S)
        pairs.append(mid(A, S, seed=80 + k))
    got, misses = check(N_MID, u, pairs)
    assert misses == [0] * 4
    assert got[3][0][0] == 0 and got[3][0][-1] == F.p - 1


def test_value_order_is_not_montgomery_limb_order():
    u = U_MID
    A, S = make_pair(90, N_MID, u, distinct=u)
    as_int = lambda v: int.from_bytes(F.to_bytes(v), "little")  # noqa: E731
    ordered = sorted(A[:u])
    assert any(as_int(a) > as_int(b) for a, b in zip(ordered, ordered[1:]))  # a sort of the stored limbs would differ
    check(N_MID, u, [(A, S)])


def test_rows_past_the_usable_ones_have_no_influence():
    """The rows >= u of A and S hold values absent from the table (as in every
    test here); replacing them changes nothing, and A' and S' receive exactly
    their n - u blinds, the input's first (asserted in check)."""
    n, u = 512, 300
    A, S = make_pair(100, n, u, distinct=40)
    got, _ = check(n, u, [(A, S)])
    other = (A[:u] + S[:n - u], S[:u] + [S[0]] * (n - u))  # table values past u in A, a usable value past u in S
    assert check(n, u, [other])[0] == got
    # a value that occurs at rows >= u of S only is missing
    late = absent(101, n, 0, S)[0]
    res, misses = check(n, u, [(A[:u - 1] + [late] + A[u:], S[:u] + [late] * (n - u)), (A, S)])
    assert misses == [1, 0] and res[0] is None and res[1] == got[0]


def test_three_lookups_of_different_content_in_one_call():
    from tachyon_amd import lookup_permute as LP
    n, u = 2048, 1500
    pairs = [make_pair(110, n, u, distinct=3), make_pair(111, n, u, distinct=u), make_pair(112, n, u, distinct=200)]
    got, misses = check(n, u, pairs)
    assert misses == [0, 0, 0]
    assert len({repeated_rows(g[0]) for g in got}) == 3
    # each lookup alone gives what it gave in the joint call
    assert check(n, u, [pairs[1]])[0] == [got[1]]
    ms = LP.last_timings()
    assert set(ms) == set(LP.PHASES) and all(v >= 0 for v in ms.values()) and ms["sort"] > 0
    assert LP.work_bytes(n, 3) > 3 * 6 * 32 * n


def test_bls12_381_fr():
    Fb = R.field("bls12_381_fr")
    n, u = N_MID, U_MID
    values = pool(120, 900, Fb)
    S = [values[k] for k in pick(121, u, 900)]
    S[3], S[5] = Fb.p - 1, 0  # p - 1: every bit of the top limb's sorted range
    A = [S[r] for r in pick(122, u, u)]
    A[0] = A[7] = Fb.p - 1
    A[1] = 0
    A, S = A + absent(123, n, u, S, Fb), S + absent(124, n, u, S, Fb)
    got, misses = check(n, u, [(A, S), make_pair(125, n, u, distinct=u, field=Fb)], field=Fb)
    assert misses == [0, 0] and got[0][0][0] == 0 and got[0][0][-2:] == [Fb.p - 1] * 2


# --- misses ----------------------------------------------------------------------------
def mid_sized(A, S, n, u):
    return A + absent(140, n, u, S), S + absent(141, n, u, S)


@pytest.mark.parametrize("where", ["below", "inside", "above"])
def test_a_missing_value(where):
    """One input value the table lacks, smaller than, inside and larger than
    the table's range: the count, the call returns, the other lookup is exact."""
    n, u = 1024, 700
    values = pool(130, 402)
    gone = {"below": values[0], "inside": values[200], "above": values[401]}[where]
    table_values = [v for v in values[1:401] if v != gone]
    S = [table_values[r] for r in pick(131, u, len(table_values))]
    A = [S[r] for r in pick(132, u, u)]
    for j in (5, 6, 300):  # the missing value three times: one distinct miss
        A[j] = gone
    good = make_pair(133, n, u, distinct=50)
    res, misses = check(n, u, [mid_sized(A, S, n, u), good])
    assert misses == [1, 0] and res[0] is None and res[1] is not None
    res, misses = check(n, u, [good, mid_sized(A, S, n, u)], seed=2)  # and in the other order
    assert misses == [0, 1] and res[0] is not None


def test_misses_with_heavy_duplication():
    """More distinct missing values than a tile has rows, in a lookup whose
    inputs repeat heavily: the leftover (R + misses values) and the repeated
    rows differ in count by more than a tile."""
    B = block()
    n, u = 4096, 3000
    values = pool(150, 2 * B + 40)
    present, gone = values[::2][:20], values[1::2][:B + 10]
    S = [present[r] for r in pick(151, u, len(present))]
    A = [present[r] for r in pick(152, u, 7)]
    for j, v in enumerate(gone):  # spread over the column; the last dozen twice
        A[3 * j] = v
    for j, v in enumerate(gone[-12:]):
        A[3 * len(gone) + j] = v
    good = make_pair(153, n, u, distinct=11)
    res, misses = check(n, u, [mid_sized(A, S, n, u), good, mid_sized(A[::-1], S, n, u)])
    assert misses == [B + 10, 0, B + 10] and res[0] is None and res[1] is not None
    # nothing of the table is asked for: every distinct input is a miss, nothing is consumed
    res, misses = check(n, u, [good, mid_sized([gone[j % len(gone)] for j in range(u)], S, n, u)], seed=3)
    assert misses == [0, B + 10] and res[0] is not None and res[1] is None


# --- into the existing path --------------------------------------------------------------
def test_device_columns_into_the_grand_product():
    """A' and S' from out= tensors go straight into lookup_grand_product: with
    random beta and gamma the product closes (the last value is 1), and with
    one element of S' altered it does not."""
    import torch
    from tachyon_amd import lookup_permute as LP
    from tachyon_amd import plonk
    n, u = 1024, 1000
    A, S = make_pair(160, n, u, distinct=300)
    dA, dS = as_cuda(R.encode(F, A)), as_cuda(R.encode(F, S))
    before = (dA.clone(), dS.clone())
    out = [tuple(torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2))]
    blinds = O.gen_scalars("bn254_fr", 161, 2 * (n - u)).tobytes()
    got = LP.permute_pairs("bn254_fr", n, u, [(dA, dS)], blinds, out=out)
    assert got is not None and got[2] == [0]
    assert torch.equal(dA, before[0]) and torch.equal(dS, before[1])  # inputs are never written
    beta, gamma = F.to_bytes(pyref.rand_scalar(162, 0, F.p)), F.to_bytes(pyref.rand_scalar(162, 1, F.p))
    z_blinds = O.gen_scalars("bn254_fr", 163, n - u - 1).tobytes()
    z = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    res = plonk.lookup_grand_product(dA, dS, out[0][0], out[0][1], beta, gamma, n, u, blinds=z_blinds, out=z)
    assert res is not None and res[1] == F.to_bytes(1)
    out[0][1][32 * 17] ^= 1  # one element of S'
    res = plonk.lookup_grand_product(dA, dS, out[0][0], out[0][1], beta, gamma, n, u, blinds=z_blinds, out=z)
    assert res is not None and res[1] != F.to_bytes(1)


def test_an_unaligned_device_column_is_staged():
    import torch
    n, u = 512, 257

    def shifted(b):
        t = torch.zeros(32 * n + 8, dtype=torch.uint8, device="cuda")
        t[8:] = as_cuda(b)
        assert t[8:].data_ptr() % 16 == 8
        return t[8:]

    check(n, u, [make_pair(170, n, u, distinct=30)], convert=shifted)


# --- refusals ------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    import ctypes

    import torch
    from tachyon_amd import lookup_permute as LP
    from tachyon_amd._lib import lib
    n, u = 16, 10
    A, S = make_pair(180, n, u, distinct=4)
    dA, dS = as_cuda(R.encode(F, A)), as_cuda(R.encode(F, S))

    def filled(rows=n):
        return torch.full((32 * rows,), 0xAB, dtype=torch.uint8, device="cuda")

    out_a, out_s = filled(), filled()
    blinds = R.encode(F, pool(181, 2 * (n - u)))
    entry = lib().tachyon_mi355x_lookup_permute_pairs
    assert LP.permute_pairs("bn254_fr", n, u, [(dA, dS)], blinds, out=[(filled(), filled())]) is not None

    def call(field=0, n_=n, u_=u, pairs=((dA, dS),), count=None, bl=blinds, a=(out_a,), s=(out_s,), null=()):
        """The C entry on device pointers; `null` names the arrays passed as null."""
        arr = (LP.LookupPair * max(1, len(pairs)))()
        for i, (x, y) in enumerate(pairs):
            arr[i].input = None if x is None else x.data_ptr()
            arr[i].table = None if y is None else y.data_ptr()
        array = ctypes.c_void_p * max(1, len(a))
        pa = array(*[None if t is None else t.data_ptr() for t in a])
        ps = array(*[None if t is None else t.data_ptr() for t in s])
        return entry(field, n_, u_, None if "pairs" in null else arr, len(pairs) if count is None else count,
                     None if "blinds" in null else bl, None if "a" in null else pa, None if "s" in null else ps, None)

    assert call(a=(filled(),), s=(filled(),)) == 1  # the call itself is good
    for field in (1, 3, -1):
        assert call(field=field) == 0
    for n_, u_ in ((12, 5), (24, 10), (1, 0), (0, 0), (n, 0), (n, n), (n, n + 1), (1 << 31, u)):
        assert call(n_=n_, u_=u_) == 0
    for null in ("pairs", "blinds", "a", "s"):
        assert call(null=(null,)) == 0
    assert call(pairs=((None, dS),)) == 0
    assert call(pairs=((dA, None),)) == 0
    assert call(a=(None,)) == 0
    assert call(s=(None,)) == 0
    assert call(s=(out_a,)) == 0  # S' is A'
    big = filled(2 * n)
    assert call(a=(big[:32 * n],), s=(big[32 * (n - 1):32 * (2 * n - 1)],)) == 0  # S' begins inside A'
    for alias in (dA, dS):  # an output that is a column of the call
        keep = alias.clone()
        assert call(a=(alias,)) == 0
        assert call(s=(alias,)) == 0
        assert torch.equal(alias, keep)
    # two pairs: an output of one is a column or an output of the other
    A2, S2 = as_cuda(R.encode(F, A)), as_cuda(R.encode(F, S))
    o2a, o2s = filled(), filled()
    two = ((dA, dS), (A2, S2))
    assert call(pairs=two, bl=blinds * 2, a=(out_a, o2a), s=(out_s, o2s)) == 1
    out_a.fill_(0xAB), out_s.fill_(0xAB), o2a.fill_(0xAB), o2s.fill_(0xAB)
    assert call(pairs=two, bl=blinds * 2, a=(out_a, out_s), s=(out_s, o2s)) == 0
    assert call(pairs=two, bl=blinds * 2, a=(out_a, o2a), s=(out_s, out_a)) == 0
    assert call(pairs=two, bl=blinds * 2, a=(out_a, o2a), s=(A2, o2s)) == 0
    # through the binding: the blind count and a null output
    assert LP.permute_pairs("bn254_fr", n, u, [(dA, dS)], blinds[32:], out=[(out_a, out_s)]) is None
    assert LP.permute_pairs("bn254_fr", n, u, [(dA, dS)], blinds + bytes(32), out=[(out_a, out_s)]) is None
    assert LP.permute_pairs("bn254_fr", n, u, [(dA, dS)], blinds, out=[(out_a, None)]) is None
    torch.cuda.synchronize()
    assert all(bool((t == 0xAB).all()) for t in (out_a, out_s, o2a, o2s, big))
    # nothing to do is no refusal
    assert LP.permute_pairs("bn254_fr", n, u, [], b"") == ([], [], [])
    assert call(pairs=(), count=0, null=("pairs", "blinds", "a", "s")) == 1
