"""The permuted lookup columns' reference module on the CPU
(tests/lookup_permute_ref.py): the reference's sequential walk, pinned by the
hand-worked cases, halo2's sanity check, the closed form the GPU path follows
and the lines of tests/quotient_ref.py that sort a duplicate-free lookup; and
the stand-alone check of the entry point's refusal rules
(tachyon_amd/csrc/check/lookup_permute_validate_check.cc), built with a plain
host compiler under the address and undefined-behaviour sanitizers.
"""
import os
import subprocess
from collections import Counter

import pytest

import lookup_permute_ref as R
from oracle import pyref

F = R.field("bn254_fr")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tachyon_amd", "csrc", "check", "lookup_permute_validate_check.cc")


def rand(seed, count):
    return [pyref.rand_scalar(seed, i, F.p) for i in range(count)]


def pair(seed, n, u, distinct=None):
    """(A, S) as canonical ints, every input from the table's usable rows;
    distinct: the table has that many different values, in no order."""
    table = rand(seed, n)
    if distinct:
        table = [table[pyref.rand_u64(seed + 1, i) % distinct] for i in range(n)]
    inputs = [table[pyref.rand_u64(seed + 2, j) % u] for j in range(n)]
    return inputs, table


def closed_form(u, A, S):
    """The result as the issue states it, with no walk: ranks and a leftover list."""
    a_perm = sorted(A[:u])
    first = [i == 0 or a_perm[i] != a_perm[i - 1] for i in range(u)]
    left = Counter(S[:u])
    left.subtract(Counter(v for i, v in enumerate(a_perm) if first[i]))
    assert min(left.values()) >= 0
    leftover = sorted(left.elements())
    repeated = [i for i in range(u) if not first[i]]
    R_ = len(repeated)
    assert len(leftover) == R_
    rank = {row: r for r, row in enumerate(repeated)}
    return a_perm, [a_perm[i] if first[i] else leftover[R_ - 1 - rank[i]] for i in range(u)]


def test_the_references_own_example():
    assert R.permute_rows(4, [1, 2, 1, 5], [1, 2, 4, 5]) == ([1, 1, 2, 5], [1, 4, 2, 5])


def test_two_repeated_rows_take_the_leftover_from_the_back():
    # leftover [1, 4]: 1 goes to row 2, 4 goes to row 1
    assert R.permute_rows(4, [1, 1, 1, 2], [1, 1, 2, 4]) == ([1, 1, 1, 2], [1, 4, 1, 2])


def test_rows_past_the_usable_ones_are_ignored_and_blinded():
    n, u = 8, 4
    A, S = [1, 2, 1, 5, 77, 78, 79, 80], [1, 2, 4, 5, 90, 91, 92, 93]
    blinds = rand(3, 2 * (n - u))
    a, s = R.permute_pair(F, n, u, R.encode(F, A), R.encode(F, S), blinds)
    assert R.decode(F, a) == [1, 1, 2, 5] + blinds[:4]
    assert R.decode(F, s) == [1, 4, 2, 5] + blinds[4:]


@pytest.mark.parametrize("distinct", [None, 1, 3, 11])
def test_halo2_sanity_check_and_multisets(distinct):
    n, u = 64, 59
    A, S = pair(10, n, u, distinct)
    a_perm, s_perm = R.permute_rows(u, A, S)
    last = None  # permute_expression_pair_unittest.cc:44-54
    for i in range(u):
        if a_perm[i] != s_perm[i]:
            assert a_perm[i] == last
        last = a_perm[i]
    assert Counter(a_perm) == Counter(A[:u]) and Counter(s_perm) == Counter(S[:u])
    assert a_perm == sorted(a_perm)
    assert a_perm[0] == s_perm[0]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("distinct", [1, 2, 7, 40])
def test_the_closed_form_is_what_the_walk_leaves(seed, distinct):
    n, u = 128, 101 + seed
    A, S = pair(20 + seed, n, u, distinct)
    assert R.permute_rows(u, A, S) == closed_form(u, A, S)


def test_a_duplicate_free_table_as_the_quotient_reference_sorts_it():
    n, u = 64, 50
    t = rand(30, n)
    inp = [t[x % u] for x in rand(31, n)]
    # tests/quotient_ref.py:348-350
    a_perm = sorted(inp[:u])
    unused = sorted(set(t[:u]) - set(a_perm))
    s_perm = [v if j == 0 or v != a_perm[j - 1] else unused.pop() for j, v in enumerate(a_perm)]
    assert R.permute_rows(u, inp, t) == (a_perm, s_perm)
    assert len(set(a_perm)) < u  # some rows repeat: the pops happened


def test_a_missing_value_returns_none():
    # the reference's second unit test: inputs 2 i, table 3 i
    n, u = 32, 27
    A, S = [2 * i for i in range(n)], [3 * i for i in range(n)]
    assert R.permute_rows(u, A, S) is None
    assert R.permute_pair(F, n, u, R.encode(F, A), R.encode(F, S), rand(40, 2 * (n - u))) is None
    assert R.misses(u, A, S) == sum(1 for i in range(u) if 2 * i % 3 or 2 * i > 3 * (u - 1))
    # a value that occurs past the usable rows only is missing too
    assert R.permute_rows(4, [1, 2, 1, 6], [1, 2, 4, 5, 6]) is None
    assert R.misses(4, [1, 2, 1, 5], [1, 2, 4, 5]) == 0


def test_validate_check_under_sanitizers(tmp_path):
    exe = tmp_path / "lookup_permute_validate_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", str(exe), CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "lookup_permute_validate_check ok" and run.stderr == "", run.stdout + run.stderr
