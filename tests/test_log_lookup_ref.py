"""The log-derivative lookup's reference module on the CPU
(tests/log_lookup_ref.py), pinned by properties of the argument and by tables
whose counted rows are worked out by hand from the bisection, and the
stand-alone check of the entry points' refusal rules
(tachyon_amd/csrc/check/log_lookup_validate_check.cc), built with a plain host
compiler under the address and undefined-behaviour sanitizers.
"""
import os
import subprocess

import pytest

import log_lookup_ref as R
from oracle import pyref

F = R.field("bn254_fr")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tachyon_amd", "csrc", "check", "log_lookup_validate_check.cc")


def rand(seed, count):
    return [pyref.rand_scalar(seed, i, F.p) for i in range(count)]


def lookup(seed, n, u, K, table_size=None):
    """A lookup whose inputs all lie in the table's usable rows: canonical ints."""
    table = rand(seed, n)
    if table_size:  # few distinct values: a table padded with duplicates
        table = [table[i % table_size] for i in range(n)]
    inputs = [[table[pyref.rand_u64(seed + 1 + k, j) % u] for j in range(n)] for k in range(K)]
    return inputs, table


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("table_size", [None, 5])
def test_a_satisfied_lookup_balances(K, table_size):
    n, u = 32, 27
    inputs, table = lookup(10 * K, n, u, K, table_size)
    counts, misses = R.m_counts(u, inputs, table)
    assert misses == 0 and sum(counts) == K * u
    m_bytes, _ = R.m_poly(F, n, u, [R.encode(F, f) for f in inputs], R.encode(F, table))
    assert R.decode(F, m_bytes) == counts + [0] * (n - u)
    blinds = rand(99, n - u - 1)
    beta = 0xBE7A
    phi, total = R.grand_sum(F, n, u, beta, [R.encode(F, f) for f in inputs], R.encode(F, table), m_bytes, blinds)
    rows = R.decode(F, phi)
    assert total == F.to_bytes(0)
    assert rows[0] == 0 and rows[u] == 0 and rows[u + 1:] == blinds
    L = R.log_derivative_terms(F, u, beta, inputs, table, counts)
    assert all((rows[i + 1] - rows[i] - L[i]) % F.p == 0 for i in range(u - 1))
    assert (rows[u - 1] + L[u - 1]) % F.p == 0  # the last step closes the sum; it is not stored


# (table, searched value, the row that is counted), each worked by hand:
#  sorted (value, row) entries, then left = 0, right = 7, mid = left + (right - left) // 2
HAND = [
    # sorted: (1,6) (3,1) (3,3) (3,5) (5,0) (7,4) (9,2); mid = 3 is (3,5): the LAST duplicate
    ([5, 3, 9, 3, 7, 3, 1], 3, 5),
    # sorted: (1,0) (2,1) (3,2) (3,3) (3,4) (8,5) (9,6); mid = 3 is (3,3): the MIDDLE duplicate
    ([1, 2, 3, 3, 3, 8, 9], 3, 3),
    # sorted: (3,0) (3,1) (3,2) (4,3) (5,4) (6,5) (7,6); mid = 3 is 4 > 3: right = 3; mid = 1 is (3,1): the middle
    ([3, 3, 3, 4, 5, 6, 7], 3, 1),
    # sorted: (1,0) (2,1) (4,2) (5,3) (6,4) (6,5) (6,6); mid = 3 is 5 < 6: left = 4; mid = 5 is (6,5): the middle
    ([1, 2, 4, 5, 6, 6, 6], 6, 5),
    # sorted: (0,3) (2,0) (2,2) (2,6) (5,1) (5,4) (5,5); 5: mid = 3 is 2 < 5: left = 4; mid = 5 is (5,4)
    ([2, 5, 2, 0, 5, 5, 2], 5, 4),
    # the same table, 2: mid = 3 is (2,6): the last of rows 0, 2, 6
    ([2, 5, 2, 0, 5, 5, 2], 2, 6),
    # all equal: sorted by row; mid = 3
    ([4, 4, 4, 4, 4, 4, 4], 4, 3),
    # 9 at rows 0 and 6 only: sorted (1,1) (2,2) (3,3) (4,4) (5,5) (9,0) (9,6); mid = 3, left = 4; mid = 5 is (9,0)
    ([9, 1, 2, 3, 4, 5, 9], 9, 0),
]


@pytest.mark.parametrize("table,value,row", HAND)
def test_hand_worked_duplicates(table, value, row):
    u, n = 7, 8
    counts, misses = R.m_counts(u, [[value] * n], table + [value])  # row 7 is no usable row
    assert misses == 0
    assert counts == [u if i == row else 0 for i in range(u)]


def test_a_value_only_past_the_usable_rows_misses():
    u = 7
    counts, misses = R.m_counts(u, [[8, 1, 8, 1, 8, 8, 8, 1]], [1, 2, 3, 4, 5, 6, 7, 8])
    assert counts == [2, 0, 0, 0, 0, 0, 0] and misses == 5


def test_misses_leave_m_untouched():
    n, u = 16, 11
    inputs, table = lookup(50, n, u, 2)
    counts, _ = R.m_counts(u, inputs, table)
    absent = [x for x in rand(51, 40) if x not in table][:n]
    with_misses, misses = R.m_counts(u, inputs + [absent], table)
    assert with_misses == counts and misses == u
    # an unbalanced lookup: the total is not 0, phi[u] still is
    enc = [R.encode(F, f) for f in inputs + [absent]]
    m_bytes, _ = R.m_poly(F, n, u, enc, R.encode(F, table))
    phi, total = R.grand_sum(F, n, u, 12345, enc, R.encode(F, table), m_bytes, rand(52, n - u - 1))
    assert total != F.to_bytes(0)
    assert R.decode(F, phi)[u] == 0 and R.decode(F, phi)[u - 1] != 0


def test_a_zero_denominator_contributes_nothing():
    n, u, beta = 8, 5, 77
    table = [1, 2, 3, 4, 5, 6, 7, 8]
    f = [1, (-beta) % F.p, 3, 3, 5, 0, 0, 0]  # row 1: f + beta = 0
    t = list(table)
    t[2] = (-beta) % F.p  # row 2: t + beta = 0, so the two lookups of 3 land elsewhere: m[2] irrelevant
    m = [1, 0, 9, 0, 1, 0, 0, 0]
    L = R.log_derivative_terms(F, u, beta, [f], t, m)
    inv = lambda x: pow(x, -1, F.p)  # noqa: E731
    assert L[1] == 0  # 0 - 0 / (2 + beta)
    assert L[2] == inv(3 + beta)  # the m term is forced to 0 whatever m is
    assert L[0] == 0 and L[4] == 0


def test_validate_check_under_sanitizers(tmp_path):
    exe = tmp_path / "log_lookup_validate_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", str(exe), CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "log_lookup_validate_check ok" and run.stderr == "", run.stdout + run.stderr
