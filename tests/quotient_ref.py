"""Pure-Python restatement of the Halo2 quotient h(X) over oracle.pyref.Field
(test infrastructure; shares no code with the product and never builds a
graph: expressions are evaluated recursively, the closed forms straight from
their formulas).

Reference: zk/plonk/vanishing/circuit_polynomial_builder.h:199-245 (parts,
order of the terms, the accumulator carried over the circuits),
custom_gate_evaluator.h (acc = acc y + poly for every gate polynomial),
permutation/permutation_evaluator.h:25-108, lookup/halo2/evaluator.h:66-128,
shuffle/evaluator.h:71-119 (with Halo2's indexing: shuffle k reads product k),
vanishing_utils.h:183-196 (ext[j P + i] = part_i[j]), :65-112 (division by
X^n - 1), :167-180 (coset IFFT, offset zeta), vanishing_prover_impl.h:106-112
(the truncation).  The oracle's NTT does the coset transforms.

A system is a dict of canonical ints:
  n, cs_degree, last_row, theta, beta, gamma, y, zeta, delta,
  l_first, l_last, l_active_row          coefficient lists (or evaluations, for `part`)
  gates        None (no gate group), [] with "empty_gates" (the empty graph: acc = 0),
               or the list of gate polynomials (expression tuples)
  perm_columns [(kind, index)], sigmas [lists]
  lookups      [(input expressions, table expressions)]
  shuffles     [(input expressions, shuffle expressions)]
  circuits     [{fixed, advice, instance: [lists], challenges: [ints], perm_z: [lists],
                 lookups: [(Z, A', S')], shuffle_z: [lists]}]
Expressions: ("const", v) ("fixed"|"advice"|"instance", column, rotation)
("challenge", i) ("neg", e) ("sum", a, b) ("product", a, b) ("scaled", e, v).
"""
from oracle import oracle as O
from oracle import pyref


def field(name="bn254_fr"):
    return pyref.Field(name)


def decode(F, col: bytes):
    rinv = pow(F.R, -1, F.p)
    return [int.from_bytes(col[k:k + 32], "little") * rinv % F.p for k in range(0, len(col), 32)]


def encode(F, xs) -> bytes:
    return b"".join(F.to_bytes(x) for x in xs)


def extended_k(n, cs_degree):
    e = n.bit_length() - 1
    while (1 << e) < n * (cs_degree - 1):
        e += 1
    return e


def get_zeta(F, vendor="scroll"):
    z = pow(F.gen, (F.p - 1) // 3, F.p)
    return z * z % F.p if vendor == "pse" else z


def domain_generator(F, size):
    """The generator the oracle's NTT uses at this size (under the active
    generator set): the evaluations of X are its powers."""
    if size == 1:
        return 1
    ev = O.fft(encode(F, [0, 1]), size, None, field=F.name)
    return decode(F, ev)[1]


# --- one row (or one point) of the numerator -------------------------------------
def eval_expr(F, e, col, challenges):
    """col(kind, index, rotation) -> the column's value at the rotated row / point."""
    p, tag = F.p, e[0]
    if tag == "const":
        return e[1] % p
    if tag in ("fixed", "advice", "instance"):
        return col(tag, e[1], e[2])
    if tag == "challenge":
        return challenges[e[1]]
    if tag == "neg":
        return -eval_expr(F, e[1], col, challenges) % p
    if tag == "sum":
        return (eval_expr(F, e[1], col, challenges) + eval_expr(F, e[2], col, challenges)) % p
    if tag == "product":
        return eval_expr(F, e[1], col, challenges) * eval_expr(F, e[2], col, challenges) % p
    if tag == "scaled":
        return eval_expr(F, e[1], col, challenges) * e[2] % p
    raise ValueError(tag)


def compress(F, S, exprs, col, challenges):
    v = 0
    for e in exprs:
        v = (v * S["theta"] + eval_expr(F, e, col, challenges)) % F.p
    return v


def gate_terms(F, S, acc, col, challenges):
    if S.get("gates") is None:
        return acc
    if S.get("empty_gates"):
        return 0
    for poly in S["gates"]:
        acc = (acc * S["y"] + eval_expr(F, poly, col, challenges)) % F.p
    return acc


def permutation_terms(F, S, acc, col, shared, zs, label):
    """shared(name, rot): l_first / l_last / l_active_row / ("sigma", i); zs(j, rot);
    label: delta_start times the row's (the point's) X, i.e. beta X."""
    p, y, m = F.p, S["y"], len(S["perm_columns"])
    if m == 0:
        return acc
    L = S["cs_degree"] - 2
    k = (m + L - 1) // L
    lf, ll, la = shared("l_first", 0), shared("l_last", 0), shared("l_active_row", 0)
    acc = (acc * y + (1 - zs(0, 0)) * lf) % p
    zl = zs(k - 1, 0)
    acc = (acc * y + ll * (zl * zl - zl)) % p
    for j in range(1, k):
        acc = (acc * y + lf * (zs(j, 0) - zs(j - 1, S["last_row"]))) % p
    cur = label
    for j in range(k):
        left, right = zs(j, 1), zs(j, 0)
        for i in range(j * L, min(m, (j + 1) * L)):
            kind, idx = S["perm_columns"][i]
            v = col(kind, idx, 0)
            left = left * (v + S["beta"] * shared(("sigma", i), 0) + S["gamma"]) % p
            right = right * (v + cur + S["gamma"]) % p
            cur = cur * S["delta"] % p
        acc = (acc * y + (left - right) * la) % p
    return acc


def lookup_terms(F, S, acc, col, challenges, shared, exprs, z, a, s):
    """z, a, s: (rot) -> the lookup's Z, A', S' at the rotated row / point."""
    p, y = F.p, S["y"]
    lf, ll, la = shared("l_first", 0), shared("l_last", 0), shared("l_active_row", 0)
    table_value = (compress(F, S, exprs[0], col, challenges) + S["beta"]) * \
                  (compress(F, S, exprs[1], col, challenges) + S["gamma"]) % p
    acc = (acc * y + lf * (1 - z(0))) % p
    acc = (acc * y + ll * (z(0) * z(0) - z(0))) % p
    acc = (acc * y + la * (z(1) * (a(0) + S["beta"]) * (s(0) + S["gamma"]) - z(0) * table_value)) % p
    acc = (acc * y + lf * (a(0) - s(0))) % p
    return (acc * y + la * (a(0) - s(0)) * (a(0) - a(-1))) % p


def shuffle_terms(F, S, acc, col, challenges, shared, exprs, z):
    p, y = F.p, S["y"]
    lf, ll, la = shared("l_first", 0), shared("l_last", 0), shared("l_active_row", 0)
    iv = (compress(F, S, exprs[0], col, challenges) + S["gamma"]) % p
    sv = (compress(F, S, exprs[1], col, challenges) + S["gamma"]) % p
    acc = (acc * y + lf * (1 - z(0))) % p
    acc = (acc * y + ll * (z(0) * z(0) - z(0))) % p
    return (acc * y + la * (z(1) * sv - z(0) * iv)) % p


def numerator(F, S, get, x, acc=0, groups=("gates", "permutation", "lookups", "shuffles")):
    """The accumulator over every circuit.  get(poly, rot): the value of a
    polynomial (a list of S, by identity) at the rotated row / point; x: the
    row's (the point's) X."""
    def shared(name, rot):
        return get(S["sigmas"][name[1]] if isinstance(name, tuple) else S[name], rot)

    for c in S["circuits"]:
        def col(kind, idx, rot, c=c):
            return get(c[kind][idx], rot)

        ch = c.get("challenges", [])
        if "gates" in groups:
            acc = gate_terms(F, S, acc, col, ch)
        if "permutation" in groups:
            acc = permutation_terms(F, S, acc, col, shared, lambda j, rot, c=c: get(c["perm_z"][j], rot),
                                    S["beta"] * x % F.p)
        if "lookups" in groups:
            for exprs, (z, a, s) in zip(S.get("lookups", []), c.get("lookups", [])):
                acc = lookup_terms(F, S, acc, col, ch, shared, exprs, lambda r, z=z: get(z, r),
                                   lambda r, a=a: get(a, r), lambda r, s=s: get(s, r))
        if "shuffles" in groups:
            for exprs, z in zip(S.get("shuffles", []), c.get("shuffle_z", [])):
                acc = shuffle_terms(F, S, acc, col, ch, shared, exprs, lambda r, z=z: get(z, r))
    return acc


def all_polys(S):
    out = [S["l_first"], S["l_last"], S["l_active_row"]] + list(S.get("sigmas", []))
    for c in S["circuits"]:
        out += list(c.get("fixed", [])) + list(c.get("advice", [])) + list(c.get("instance", []))
        out += list(c.get("perm_z", [])) + [x for t in c.get("lookups", []) for x in t] + list(c.get("shuffle_z", []))
    return [p for p in out if p is not None]


def part(F, S, x_of_row, acc, groups):
    """One coset's rows with the lists of S read as evaluations: the
    accumulator after `groups`, from the accumulator `acc`."""
    n = S["n"]
    return [numerator(F, S, lambda poly, rot, j=j: poly[(j + rot) % n], x_of_row(j), acc[j], groups)
            for j in range(n)]


def h_poly(F, S):
    """(the n (cs_degree - 1) coefficients, all n P coefficients, w_ext)."""
    n, p = S["n"], F.p
    log_ext = extended_k(n, S["cs_degree"])
    N = 1 << log_ext
    P = N // n
    w_ext = domain_generator(F, N)
    omega = pow(w_ext, P, p)
    assert n == 1 or domain_generator(F, n) == omega
    polys = all_polys(S)
    ext = [0] * N
    for i in range(P):
        h = S["zeta"] * pow(w_ext, i, p) % p
        cosets = {id(q): decode(F, O.fft(encode(F, q), n, F.to_bytes(h), field=F.name)) for q in polys}
        t_inv = pow((pow(S["zeta"], n, p) * pow(w_ext, n * i, p) - 1) % p, -1, p)
        xs = [h]
        for _ in range(n - 1):
            xs.append(xs[-1] * omega % p)
        for j in range(n):
            v = numerator(F, S, lambda poly, rot, j=j: cosets[id(poly)][(j + rot) % n], xs[j])
            ext[j * P + i] = v * t_inv % p
    coeffs = decode(F, O.ifft(encode(F, ext), N, F.to_bytes(S["zeta"]), field=F.name))
    coeffs += [0] * (N - len(coeffs))  # the oracle drops trailing zero coefficients
    return coeffs[:n * (S["cs_degree"] - 1)], coeffs, w_ext


def horner(F, coeffs, x):
    v = 0
    for c in reversed(coeffs):
        v = (v * x + c) % F.p
    return v


def identity_at(F, S, omega, h_coeffs, x):
    """numerator(x) == h(x) (x^n - 1), every polynomial evaluated at x omega^r by Horner."""
    def get(poly, rot):
        return horner(F, poly, x * pow(omega, rot % S["n"], F.p) % F.p)

    return numerator(F, S, get, x) == horner(F, h_coeffs, x) * (pow(x, S["n"], F.p) - 1) % F.p


def walk_graph(F, g, S, c, get, prev):
    """The value of a hand-written graph (a plonk_quotient.GraphEvaluator: the
    tests' op, rotation, slot and Horner cases have no expression form) by the
    reference's rule, graph_evaluator.h:60-76 and calculation.h:71-104: every
    calculation in order into its own intermediate, the last one's the value,
    zero for none."""
    p, inter = F.p, []

    def val(s):
        kind, idx, rot = s
        if kind == 0:
            return g.constants[idx]
        if kind == 1:
            return inter[idx]
        if kind in (2, 3, 4):
            return get(c[("fixed", "advice", "instance")[kind - 2]][idx], g.rotations[rot])
        if kind == 5:
            return c["challenges"][idx]
        return (S["beta"], S["gamma"], S["theta"], S["y"], prev)[kind - 6]

    for op, a, b, parts in g.calculations:
        if op == 6:
            v, f = val(a), val(b)
            for part in parts:
                v = (v * f + val(part)) % p
        else:
            x = val(a)
            if op < 3:
                w = val(b)
                v = (x + w, x - w, x * w)[op] % p
            else:
                v = {3: x * x, 4: 2 * x, 5: -x, 7: x}[op] % p
        inter.append(v)
    return inter[-1] if inter else 0


# --- systems for the tests ----------------------------------------------------------
def rand(seed, count, F):
    return [pyref.rand_scalar(seed, i, F.p) for i in range(count)]


def interpolate(F, evals):
    coeffs = decode(F, O.ifft(encode(F, evals), len(evals), None, field=F.name))
    return coeffs + [0] * (len(evals) - len(coeffs))  # the oracle drops trailing zero coefficients


def indicators(F, n, u):
    """l_first, l_last, l_active_row as coefficient lists (proving_key.h:114-166)."""
    return (interpolate(F, [1] + [0] * (n - 1)), interpolate(F, [0] * u + [1] + [0] * (n - u - 1)),
            interpolate(F, [1] * u + [0] * (n - u)))


GATE_POLYS = [
    ("product", ("fixed", 0, 0), ("sum", ("product", ("advice", 0, 0), ("advice", 1, 0)), ("neg", ("advice", 2, 0)))),
    ("sum", ("scaled", ("advice", 0, 1), 7), ("product", ("instance", 0, -1), ("challenge", 0))),
    ("product", ("sum", ("advice", 1, 0), ("const", 2)), ("sum", ("advice", 1, 0), ("const", 2))),
]
LOOKUP_EXPRS = ([("advice", 0, 0), ("product", ("fixed", 0, 0), ("advice", 1, 1))], [("fixed", 1, 0), ("instance", 0, 0)])
SHUFFLE_EXPRS = ([("advice", 2, 0)], [("sum", ("advice", 0, 0), ("fixed", 1, -1))])


def random_system(F, n, cs_degree, num_circuits=1, seed=1, perm_m=None, num_lookups=1, num_shuffles=1, u=None):
    """Random (unsatisfied) polynomials of every kind: 2 fixed, 3 advice, 1 instance per circuit."""
    L = cs_degree - 2
    m = L + 1 if perm_m is None else perm_m
    u = n - 3 if u is None else u
    it = iter(range(seed * 1000, seed * 1000 + 999))
    col = lambda: rand(next(it), n, F)
    scalars = rand(seed * 1000 + 999, 6, F)
    pool = [("fixed", 0), ("advice", 0), ("instance", 0), ("advice", 2), ("fixed", 1), ("advice", 1)]
    S = dict(n=n, cs_degree=cs_degree, last_row=u - n, theta=scalars[0], beta=scalars[1], gamma=scalars[2],
             y=scalars[3], zeta=get_zeta(F), delta=scalars[4], l_first=col(), l_last=col(), l_active_row=col(),
             gates=GATE_POLYS, perm_columns=[pool[i % len(pool)] for i in range(m)], sigmas=[col() for _ in range(m)],
             lookups=[LOOKUP_EXPRS, (LOOKUP_EXPRS[1], LOOKUP_EXPRS[0])][:num_lookups],
             shuffles=[SHUFFLE_EXPRS, (SHUFFLE_EXPRS[1], SHUFFLE_EXPRS[0])][:num_shuffles], circuits=[])
    for _ in range(num_circuits):
        S["circuits"].append(dict(fixed=[col(), col()], advice=[col(), col(), col()], instance=[col()],
                                  challenges=[scalars[5]], perm_z=[col() for _ in range((m + L - 1) // L)],
                                  lookups=[(col(), col(), col()) for _ in range(num_lookups)],
                                  shuffle_z=[col() for _ in range(num_shuffles)]))
    return S


def grand_product(F, n, u, num, den, blinds):
    """z[0] = 1, z[j+1] = z[j] num[j] / den[j] for j < u, then the blinds."""
    z = [1]
    for j in range(u):
        z.append(z[j] * num[j] % F.p * pow(den[j], -1, F.p) % F.p)
    return z + list(blinds)


def satisfied_system(F, n, u, omega, sigma_evals, witness, cs_degree, perm_z_evals=None, seed=5):
    """A toy circuit every constraint of which holds (evaluation form inside,
    coefficient form in the result): the gate s (a b - c) with s fixed and
    a, b random; the permutation over `sigma_evals` with the cycle-constant
    `witness` columns spread over fixed, advice and instance; a one-column
    lookup whose permuted pair is sorted here; one shuffle.  perm_z_evals:
    the permutation's Z columns when the caller has them (else computed
    here).  Returns (system, evaluation-form columns by name)."""
    p, m, L = F.p, len(sigma_evals), cs_degree - 2
    it = iter(range(seed * 1000, seed * 1000 + 999))
    col = lambda: rand(next(it), n, F)
    scalars = rand(seed * 1000 + 999, 5, F)
    theta, beta, gamma, y, delta = scalars[0], scalars[1], scalars[2], scalars[3], None
    s = [1 + x % 5 if j < u else 0 for j, x in enumerate(col())]
    a, b = col(), col()
    c = [a[j] * b[j] % p if j < u else x for j, x in enumerate(col())]
    # lookup: table t (fixed) with distinct usable rows, input picks from it
    t = col()
    inp = [t[x % u] if j < u else x for j, x in enumerate(col())]
    a_perm = sorted(inp[:u])
    unused = sorted(set(t[:u]) - set(a_perm))
    s_perm = [v if j == 0 or v != a_perm[j - 1] else unused.pop() for j, v in enumerate(a_perm)]
    a_perm, s_perm = a_perm + rand(next(it), n - u, F), s_perm + rand(next(it), n - u, F)
    lz = grand_product(F, n, u, [(inp[j] + beta) * (t[j] + gamma) % p for j in range(u)],
                       [(a_perm[j] + beta) * (s_perm[j] + gamma) % p for j in range(u)], rand(next(it), n - u - 1, F))
    # shuffle: sh is a rotation of the input over the usable rows
    sin = col()
    sh = [sin[(j + 3) % u] if j < u else x for j, x in enumerate(col())]
    sz = grand_product(F, n, u, [(sin[j] + gamma) % p for j in range(u)], [(sh[j] + gamma) % p for j in range(u)],
                       rand(next(it), n - u - 1, F))
    # the permutation's columns over the three kinds
    kinds = ["fixed", "advice", "instance"]
    table = dict(fixed=[s, t], advice=[a, b, c, inp, sin, sh], instance=[])
    perm_columns = []
    for i in range(m):
        table[kinds[i % 3]].append(witness[i])
        perm_columns.append((kinds[i % 3], len(table[kinds[i % 3]]) - 1))
    delta = pow(7, 1 << 28, p) if F.name == "bn254_fr" else pow(F.gen, 1 << 32, p)
    if perm_z_evals is None:
        perm_z_evals, last = [], 1
        for lo in range(0, m, L):
            idx = range(lo, min(m, lo + L))
            num, den = [1] * u, [1] * u
            for i in idx:
                lab = pow(delta, i, p)
                for j in range(u):
                    num[j] = num[j] * (witness[i][j] + beta * lab + gamma) % p
                    den[j] = den[j] * (witness[i][j] + beta * sigma_evals[i][j] + gamma) % p
                    lab = lab * omega % p
            z = grand_product(F, n, u, num, den, rand(next(it), n - u - 1, F))
            z = [x * last % p for x in z[:u + 1]] + z[u + 1:]
            last = z[u]
            perm_z_evals.append(z)
    I = lambda ev: interpolate(F, ev)
    lf, ll, la = indicators(F, n, u)
    gate = ("product", ("fixed", 0, 0), ("sum", ("product", ("advice", 0, 0), ("advice", 1, 0)), ("neg", ("advice", 2, 0))))
    S = dict(n=n, cs_degree=cs_degree, last_row=u - n, theta=theta, beta=beta, gamma=gamma, y=y, zeta=get_zeta(F),
             delta=delta, l_first=lf, l_last=ll, l_active_row=la, gates=[gate], perm_columns=perm_columns,
             sigmas=[I(x) for x in sigma_evals], lookups=[([("advice", 3, 0)], [("fixed", 1, 0)])],
             shuffles=[([("advice", 4, 0)], [("advice", 5, 0)])],
             circuits=[dict(fixed=[I(x) for x in table["fixed"]], advice=[I(x) for x in table["advice"]],
                            instance=[I(x) for x in table["instance"]], challenges=[],
                            perm_z=[I(x) for x in perm_z_evals], lookups=[(I(lz), I(a_perm), I(s_perm))],
                            shuffle_z=[I(sz)])])
    return S


# --- the library's call for a system -------------------------------------------------
def graph_of(field_name, kind, exprs):
    from tachyon_amd.plonk_quotient import GraphEvaluator
    if kind == "gates":
        return GraphEvaluator.for_gates(exprs, field_name)
    if kind == "lookup":
        return GraphEvaluator.for_lookup(exprs[0], exprs[1], field_name)
    return GraphEvaluator.for_shuffle(exprs[0], exprs[1], field_name)


def library_kwargs(F, S, conv=None):
    """(circuits, keyword arguments) of plonk_quotient.quotient_h_poly /
    quotient_work_bytes for the system S; conv(bytes) places a polynomial
    (identity: host bytes)."""
    from tachyon_amd.plonk_quotient import GraphEvaluator
    conv = conv or (lambda b: b)
    cache = {}

    def poly(xs):
        if id(xs) not in cache:
            cache[id(xs)] = conv(encode(F, xs))
        return cache[id(xs)]

    gates = None
    if S.get("gates") is not None:
        gates = GraphEvaluator(F.name) if S.get("empty_gates") else graph_of(F.name, "gates", S["gates"])
    circuits = [dict(fixed=[poly(x) for x in c["fixed"]], advice=[poly(x) for x in c["advice"]],
                     instance=[poly(x) for x in c["instance"]], challenges=[F.to_bytes(x) for x in c["challenges"]],
                     perm_z=[poly(x) for x in c["perm_z"]], lookups=[tuple(poly(x) for x in t) for t in c["lookups"]],
                     shuffle_z=[poly(x) for x in c["shuffle_z"]]) for c in S["circuits"]]
    kw = dict(cs_degree=S["cs_degree"], last_row=S["last_row"], theta=F.to_bytes(S["theta"]), beta=F.to_bytes(S["beta"]),
              gamma=F.to_bytes(S["gamma"]), y=F.to_bytes(S["y"]), l_first=poly(S["l_first"]), l_last=poly(S["l_last"]),
              l_active_row=poly(S["l_active_row"]), gates=gates, perm_columns=S["perm_columns"],
              sigmas=[poly(x) for x in S["sigmas"]], lookups=[graph_of(F.name, "lookup", e) for e in S["lookups"]],
              shuffles=[graph_of(F.name, "shuffle", e) for e in S["shuffles"]])
    return circuits, kw
