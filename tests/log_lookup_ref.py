"""Pure-Python restatement of the log-derivative lookup's two prover steps over
oracle.pyref.Field (test infrastructure; shares no code with the product).

Reference: tachyon/zk/lookup/log_derivative_halo2/prover_impl.h
  ComputeMPoly (:99-140): the entries (i, table[i].ToBigInt()), i < usable
    rows, go through base::StableSort by the integer alone; every input value
    of every input column at the rows < usable rows is searched with
    base::BinarySearchByKey (base/containers/container_util.h:169-185), which
    returns the FIRST position its bisection finds equal; a hit adds 1 to the
    counter of that entry's original row, a miss nothing; m = the counters,
    zero from the usable rows on.
  CreateGrandSumPoly (:186-298): L[i] = sum_k 1 / (f_k[i] + beta) -
    m[i] / (t[i] + beta) with the batch inverse's rule that a zero stays zero
    (math/base/groups.h:124-143); phi[0] = 0, phi[i] = L[0] + .. + L[i-1] for
    i < usable rows; phi[usable rows] = 0 (the vector is zero-initialised and
    the sums stop one row short); Blinder::Blind over the last n - usable rows
    - 1 rows (zk/base/blinder.h:33-45).
Columns are Montgomery bytes of n elements; results are canonical Montgomery
bytes.
"""
from grand_product_ref import decode, encode, field  # noqa: F401  (re-exported for the tests)


def binary_search_by_key(keys, x):
    """BinarySearchByKey: the position of the first equal key the bisection
    meets, or None."""
    left, right = 0, len(keys)
    while left < right:
        mid = left + (right - left) // 2
        if keys[mid] < x:
            left = mid + 1
        elif x < keys[mid]:
            right = mid
        else:
            return mid
    return None


def m_counts(u, inputs, table):
    """(counters of the rows < u, misses) over canonical ints."""
    order = sorted(range(u), key=lambda i: table[i])  # stable: ties keep ascending i
    keys = [table[i] for i in order]
    counts, misses = [0] * u, 0
    for f in inputs:
        for j in range(u):
            at = binary_search_by_key(keys, f[j])
            if at is None:
                misses += 1
            else:
                counts[order[at]] += 1
    return counts, misses


def m_poly(F, n, u, inputs, table):
    """(m as bytes, misses) of one lookup; inputs: a list of columns."""
    assert 0 < u < n
    counts, misses = m_counts(u, [decode(F, bytes(f)) for f in inputs], decode(F, bytes(table)))
    return encode(F, counts + [0] * (n - u)), misses


def inverse_or_zero(F, x):
    return pow(x, -1, F.p) if x % F.p else 0


def log_derivative_terms(F, u, beta, inputs, table, m):
    """L[0..u) over canonical ints."""
    out = []
    for i in range(u):
        s = sum(inverse_or_zero(F, (f[i] + beta) % F.p) for f in inputs)
        out.append((s - m[i] * inverse_or_zero(F, (table[i] + beta) % F.p)) % F.p)
    return out


def grand_sum(F, n, u, beta, inputs, table, m, blinds):
    """(phi as bytes, the sum of L over all u rows as bytes) of one lookup.
    beta: a canonical int; blinds: n - u - 1 canonical ints."""
    assert 0 < u < n and len(blinds) == n - u - 1
    L = log_derivative_terms(F, u, beta, [decode(F, bytes(f)) for f in inputs], decode(F, bytes(table)),
                             decode(F, bytes(m)))
    phi, acc = [], 0
    for i in range(u):
        phi.append(acc)
        acc = (acc + L[i]) % F.p
    return encode(F, phi + [0] + list(blinds)), F.to_bytes(acc)
