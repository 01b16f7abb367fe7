"""Pure-Python restatement of the Halo2 lookup's permuted columns over
oracle.pyref.Field (test infrastructure; shares no code with the product).

Reference: tachyon/zk/lookup/halo2/permute_expression_pair.h:29-142
(PermuteExpressionPair), restated step for step, the sequential walk included:
  the input's usable rows are sorted by value (operator< of the prime field
    compares the canonical integers, prime_field_fallback.h:182-184; the sort
    is unstable, and equal values are equal bytes);
  a map from each table value of the usable rows to its count;
  over the sorted rows: row 0 and every row that differs from the one before
    it takes its own value into S' and one instance of it out of the map (a
    value the map does not have: the reference returns false, PermutePair
    CHECK-aborts); every other row is pushed on repeated_input_rows;
  the map's remaining values, in ascending order and each as often as its
    count says, go to repeated_input_rows.back(), which is then popped;
  both columns are blinded with include_last_row = true (zk/base/blinder.h:
    33-45): the rows from usable_rows on, n - usable_rows values each, the
    input's before the table's (lookup/halo2/prover_impl.h:74-95).

The reference's own example, u = 4:
    A = [1, 2, 1, 5], S = [1, 2, 4, 5]  ->  A' = [1, 1, 2, 5], S' = [1, 4, 2, 5]
and one with two repeated rows, where the leftover is [1, 4]: 1, the smaller,
goes to the last repeated row (2), 4 to row 1:
    A = [1, 1, 1, 2], S = [1, 1, 2, 4]  ->  A' = [1, 1, 1, 2], S' = [1, 4, 1, 2]

Columns are Montgomery bytes of n elements; results are canonical Montgomery
bytes (the elements of a column the tests encode are canonical already, so
these are the bytes they came in with).
"""
from grand_product_ref import decode, encode, field  # noqa: F401  (re-exported for the tests)


def permute_rows(u, inputs, table):
    """(A'[0..u), S'[0..u)) over canonical ints, or None when an input value is
    missing from the table's usable rows."""
    permuted_input = sorted(inputs[:u])
    leftover_table_map = {}
    for i in range(u):
        coeff = table[i]
        if coeff not in leftover_table_map:
            leftover_table_map[coeff] = 1
        else:
            leftover_table_map[coeff] += 1
    permuted_table = [None] * u
    repeated_input_rows = []
    for row in range(u):
        input_value = permuted_input[row]
        if row == 0 or input_value != permuted_input[row - 1]:
            permuted_table[row] = input_value
            if input_value not in leftover_table_map:
                return None
            assert leftover_table_map[input_value] > 0
            leftover_table_map[input_value] -= 1
        else:
            repeated_input_rows.append(row)
    for coeff in sorted(leftover_table_map):  # a btree_map iterates in key order
        for _ in range(leftover_table_map[coeff]):
            assert repeated_input_rows
            permuted_table[repeated_input_rows.pop()] = coeff
    assert not repeated_input_rows
    return permuted_input, permuted_table


def misses(u, inputs, table):
    """The distinct values of the input's usable rows that the table's usable rows lack."""
    return len(set(inputs[:u]) - set(table[:u]))


def permute_pair(F, n, u, A, S, blinds):
    """(A' as bytes, S' as bytes) of one lookup, or None on a missing value.
    blinds: 2 (n - u) canonical ints, those of A' first."""
    assert 0 < u < n and len(blinds) == 2 * (n - u)
    rows = permute_rows(u, decode(F, bytes(A)), decode(F, bytes(S)))
    if rows is None:
        return None
    return encode(F, rows[0] + list(blinds[:n - u])), encode(F, rows[1] + list(blinds[n - u:]))
