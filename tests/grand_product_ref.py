"""Pure-Python restatement of the Halo2 grand-product polynomials over
oracle.pyref.Field (test infrastructure; shares no code with the product).

Reference: tachyon/zk/plonk/permutation/grand_product_argument.h:17-122 --
ratio(j) = numerator(j) * BatchInverse(denominator)(j), a zero denominator's
inverse being 0 (math/base/groups.h:124-180); DoCreatePoly: z[0] = last_z,
z[j+1] = z[j] ratio(j) for j < usable_rows, last_z = z[usable_rows]; then
Blinder::Blind over the last n - usable_rows - 1 rows (zk/base/blinder.h:
33-45) -- and the three callback pairs:
  permutation  permutation_prover_impl.h:216-244 over the column chunks of
               :24-86, labels delta^i omega^j (unpermuted_table.h:55-79),
               chunk length cs_degree - 2 and delta (permutation_utils.h:12-35)
  lookup       lookup/halo2/prover_impl.h:126-138
  shuffle      shuffle/prover_impl.h:77
Jobs and factors have the shape tachyon_amd.plonk takes: a factor is a dict
{values, m, table, label, c} (values / table: Montgomery bytes of n elements,
m / c: Montgomery bytes or None), a job (numerator list, denominator list), a
chain a list of jobs.  Results are canonical Montgomery bytes.
"""
from oracle import pyref

from tachyon_amd import params as P


def field(name="bn254_fr"):
    return pyref.Field(name)


def get_delta(F) -> int:
    """GetDelta: g^(2^s); BN254's pinned constant is 7^(2^28)."""
    if F.name == "bn254_fr":
        return pow(7, 1 << 28, F.p)
    return pow(F.gen, 1 << P.two_adicity(F.p), F.p)


def factor(values, m=None, table=None, label=None, c=None):
    return {"values": values, "m": m, "table": table, "label": label, "c": c}


def decode(F, col: bytes):
    rinv = pow(F.R, -1, F.p)
    return [int.from_bytes(col[k:k + 32], "little") * rinv % F.p for k in range(0, len(col), 32)]


def encode(F, xs) -> bytes:
    return b"".join(F.to_bytes(x) for x in xs)


def _side(F, factors, rows, omega, delta, cols):
    out = [1] * rows
    for f in factors:
        v = cols(f["values"])
        m = F.from_bytes(f["m"]) if f["m"] is not None else 0
        c = F.from_bytes(f["c"]) if f["c"] is not None else 0
        if f["table"] is not None:
            t = cols(f["table"])
        elif f["label"] is not None:
            t, x = [], pow(delta, f["label"], F.p)
            for _ in range(rows):
                t.append(x)
                x = x * omega % F.p
        else:
            t = None
        for j in range(rows):
            out[j] = out[j] * ((v[j] + (m * t[j] if t is not None else 0) + c) % F.p) % F.p
    return out


def grand_product_chains(F, n, u, chains, omega, delta, blinds):
    """(per job Z bytes, per chain last value bytes).  omega, delta: canonical
    ints; blinds: per job (over all chains in order) n - u - 1 canonical ints."""
    assert 0 <= u < n
    cache = {}

    def cols(b):
        if id(b) not in cache:
            cache[id(b)] = decode(F, bytes(b))
            assert len(cache[id(b)]) == n
        return cache[id(b)]

    z_all, last_all, job_index = [], [], 0
    for chain in chains:
        last = 1
        for num, den in chain:
            nv = _side(F, num, u, omega, delta, cols)
            dv = _side(F, den, u, omega, delta, cols)
            z = [last]
            for j in range(u):
                ratio = nv[j] * pow(dv[j], -1, F.p) % F.p if dv[j] else 0
                z.append(z[j] * ratio % F.p)
            last = z[u]
            bl = blinds[job_index]
            assert len(bl) == n - u - 1
            z_all.append(encode(F, z + list(bl)))
            job_index += 1
        last_all.append(F.to_bytes(last))
    return z_all, last_all


def permutation_chains(values, sigmas, beta, gamma, cs_degree):
    """Per circuit one chain over the column chunks of length cs_degree - 2."""
    L = cs_degree - 2
    assert L >= 1
    chains = []
    for cols in values:
        assert len(cols) == len(sigmas)
        chain = []
        for s in range(0, len(cols), L):
            idx = range(s, min(len(cols), s + L))
            chain.append(([factor(cols[i], m=beta, label=i, c=gamma) for i in idx],
                          [factor(cols[i], m=beta, table=sigmas[i], c=gamma) for i in idx]))
        chains.append(chain)
    return chains


def lookup_job(A, S, A_perm, S_perm, beta, gamma):
    return ([factor(A, c=beta), factor(S, c=gamma)], [factor(A_perm, c=beta), factor(S_perm, c=gamma)])


def shuffle_job(A, S, gamma):
    return ([factor(A, c=gamma)], [factor(S, c=gamma)])


# --- the golden circuits' permutations ---------------------------------------
def decode_sigmas(F, sigma_cols, omega, delta):
    """sigma_cols[i][j] (canonical ints) as cells (i', j') with
    sigma_i[j] = delta^i' omega^j'; raises KeyError on a value that is no label."""
    m, n = len(sigma_cols), len(sigma_cols[0])
    label = {}
    for i in range(m):
        x = pow(delta, i, F.p)
        for j in range(n):
            label[x] = (i, j)
            x = x * omega % F.p
    assert len(label) == m * n
    return [[label[s] for s in col] for col in sigma_cols]


def cycles(cells):
    """The cycles of the permutation (i, j) -> cells[i][j]."""
    seen, out = set(), []
    for i in range(len(cells)):
        for j in range(len(cells[i])):
            if (i, j) in seen:
                continue
            cyc, at = [], (i, j)
            while at not in seen:
                seen.add(at)
                cyc.append(at)
                at = cells[at[0]][at[1]]
            out.append(cyc)
    return out


def cycle_constant_witness(F, cells, seed):
    """Per-column values (canonical ints) constant on every cycle."""
    m, n = len(cells), len(cells[0])
    w = [[0] * n for _ in range(m)]
    for k, cyc in enumerate(cycles(cells)):
        v = pyref.rand_scalar(seed, k, F.p)
        for i, j in cyc:
            w[i][j] = v
    return w
