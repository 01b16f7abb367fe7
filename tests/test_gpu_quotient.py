"""The Halo2 quotient on the GPU (tachyon_amd.plonk_quotient over
tachyon_mi355x_quotient_*) against tests/quotient_ref.py, bytewise.

The boundaries come from the library: T = tile_rows() (rows of a workgroup:
sizes below a wave, one tile, two tiles), S = fast_slots() (intermediates in
LDS: chains built to need S-1, S, S+1 and 2S+3 live slots cross into the
spill workspace).
"""
import functools

import pytest

import grand_product_ref as G
import halo2_golden as H
import quotient_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F = H.FR
FB = R.field("bls12_381_fr")


def Q():
    from tachyon_amd import plonk_quotient
    return plonk_quotient


def T():
    return Q().tile_rows()


def fr(x, field=F):
    return field.to_bytes(x)


def cuda(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


# --- one term group on caller-held evaluations --------------------------------------
def table_system(n, seed=1, field=F, u=None):
    """Random evaluations: 2 fixed, 3 advice, 1 instance, 1 challenge; no closed-form group."""
    S = R.random_system(field, n, 4, seed=seed, perm_m=0, num_lookups=0, num_shuffles=0, u=u)
    S["gates"] = None
    return S


def run_gates(S, g, acc, field=F, c=0, conv=None):
    """quotient_evaluate_part(GATES) of the hand-written graph g on circuit c of S."""
    conv = conv or (lambda b: b)
    ci = S["circuits"][c]
    enc = lambda cols: [conv(R.encode(field, x)) for x in cols]
    return Q().quotient_evaluate_part(
        field.name, S["n"], Q().GATES, R.encode(field, acc), theta=fr(S["theta"], field), beta=fr(S["beta"], field),
        gamma=fr(S["gamma"], field), y=fr(S["y"], field), fixed=enc(ci["fixed"]), advice=enc(ci["advice"]),
        instance=enc(ci["instance"]), challenges=[fr(x, field) for x in ci["challenges"]], graph=g)


def want_gates(S, g, acc, field=F, c=0):
    n, ci = S["n"], S["circuits"][c]
    return R.encode(field, [R.walk_graph(field, g, S, ci, lambda col, rot, j=j: col[(j + rot) % n], acc[j])
                            for j in range(n)])


def check_gates(S, g, seed=9, field=F):
    acc = R.rand(seed, S["n"], field)
    got = run_gates(S, g, acc, field)
    assert got is not None and got == want_gates(S, g, acc, field)


SOURCES = {
    "constant": lambda q: (q.CONSTANT, 3, 0), "fixed": lambda q: (q.FIXED, 1, 0), "advice": lambda q: (q.ADVICE, 2, 0),
    "instance": lambda q: (q.INSTANCE, 0, 0), "challenge": lambda q: (q.CHALLENGE, 0, 0), "beta": lambda q: (q.BETA, 0, 0),
    "gamma": lambda q: (q.GAMMA, 0, 0), "theta": lambda q: (q.THETA, 0, 0), "y": lambda q: (q.Y, 0, 0),
    "previous": lambda q: (q.PREVIOUS_VALUE, 0, 0), "intermediate": lambda q: (q.INTERMEDIATE, 0, 0),
}


def fresh_graph(field=F):
    g = Q().GraphEvaluator(field.name)
    g.add_constant(0xC0FFEE)
    g.add_rotation(0)
    g.add_calculation(Q().MUL, (Q().ADVICE, 0, 0), (Q().FIXED, 0, 0))  # intermediate 0
    return g


@pytest.mark.parametrize("rows", ["8", "T"])
def test_every_op_and_source_kind(rows):
    q, n = Q(), eval(rows, {"T": T()})
    S = table_system(n)
    for op in (q.ADD, q.SUB, q.MUL, q.SQUARE, q.DOUBLE, q.NEGATE, q.STORE):
        for left, right in (("advice", "fixed"), ("previous", "y"), ("intermediate", "constant")):
            g = fresh_graph()
            g.add_calculation(op, SOURCES[left](q), SOURCES[right](q) if op <= q.MUL else None)
            check_gates(S, g)
    for name, src in SOURCES.items():
        g = fresh_graph()
        g.add_calculation(q.SUB, src(q), (q.ADVICE, 1, 0))
        check_gates(S, g)
        g = fresh_graph()
        g.add_calculation(q.HORNER, src(q), src(q), [src(q), (q.ADVICE, 1, 0)])
        check_gates(S, g)


@pytest.mark.parametrize("rows", ["8", "64", "T", "2*T"])
def test_rotations(rows):
    q, n = Q(), eval(rows, {"T": T()})
    u = n - 3
    S = table_system(n, seed=2, u=u)
    S["circuits"][0]["advice"][0] = list(range(n))  # every wrong wrap lands on another value
    rots = [0, 1, -1, 2, -(u + 1), T(), -T(), n - 1, n + 3, -(n + 3)]
    for kind, col in ((q.ADVICE, 0), (q.FIXED, 1), (q.INSTANCE, 0)):
        g = q.GraphEvaluator(F.name)
        parts = [g.add_calculation(q.STORE, (kind, col, g.add_rotation(r))) for r in rots]
        g.add_calculation(q.HORNER, (q.PREVIOUS_VALUE, 0, 0), (q.Y, 0, 0), parts)
        check_gates(S, g)
    # the row index alone, one rotation at a time: the exact rows
    for r in rots:
        g = q.GraphEvaluator(F.name)
        g.add_calculation(q.STORE, (q.ADVICE, 0, g.add_rotation(r)))
        got = run_gates(S, g, [0] * n)
        assert R.decode(F, got) == [(j + r) % n for j in range(n)], r


def chain_graph(live):
    """`live` sums all defined before the first is read, then multiplied
    together: exactly `live` values live at once; folded into the accumulator."""
    q = Q()
    g = q.GraphEvaluator(F.name)
    g.add_rotation(0), g.add_rotation(1)
    vals = [g.add_calculation(q.ADD, (q.ADVICE, i % 3, i % 2), g.add_constant(1000 + i)) for i in range(live)]
    r = vals[0]
    for v in vals[1:]:
        r = g.add_calculation(q.MUL, r, v)
    g.add_calculation(q.HORNER, (q.PREVIOUS_VALUE, 0, 0), (q.Y, 0, 0), [r])
    return g


@pytest.mark.parametrize("live", ["S-1", "S", "S+1", "2*S+3"])
def test_live_slots_around_the_lds_budget(live):
    n = 2 * T()
    k = eval(live, {"S": Q().fast_slots()})
    S = R.random_system(F, n, 4, num_circuits=2, seed=4, perm_m=0, num_lookups=0, num_shuffles=0)
    g = chain_graph(k)
    acc = R.rand(11, n, F)
    first = run_gates(S, g, acc, c=0)
    assert first == want_gates(S, g, acc, c=0)
    if live == "2*S+3":  # a second circuit: the accumulator carries
        second = run_gates(S, g, R.decode(F, first), c=1)
        assert second == want_gates(S, g, R.decode(F, first), c=1) and second != first


@pytest.mark.parametrize("count", [0, 1, 40])
def test_horner(count):
    q = Q()
    S = table_system(T(), seed=5)
    for init, factor in (((q.PREVIOUS_VALUE, 0, 0), (q.Y, 0, 0)), ((q.CONSTANT, 0, 0), (q.THETA, 0, 0))):
        g = q.GraphEvaluator(F.name)
        g.add_rotation(0), g.add_rotation(-1)
        parts = [g.add_calculation(q.ADD, (q.ADVICE, i % 3, i % 2), g.add_constant(77 + i)) for i in range(count)]
        g.add_calculation(q.HORNER, init, factor, parts)
        check_gates(S, g)


def test_empty_graph_is_zero():
    S = table_system(64, seed=6)
    g = Q().GraphEvaluator(F.name)
    got = run_gates(S, g, R.rand(12, 64, F))
    assert got == R.encode(F, [0] * 64)
    cu = run_gates(S, g, R.rand(12, 64, F), conv=cuda)
    assert cu == got


def cuda_off_by_4(b):
    """A CUDA tensor holding b that starts 4 bytes past a 16-byte boundary."""
    import torch
    view = torch.empty(len(b) + 16, dtype=torch.uint8, device="cuda")[4:4 + len(b)]
    view.copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("acc_on", ["host", "cuda"])
def test_staged_columns_and_accumulator(acc_on):
    """What the kernel cannot use in place is staged: one host object as a
    fixed and as an advice column, a device column and a device accumulator
    that are not 16-byte aligned."""
    q, n = Q(), 8
    S = table_system(n, seed=7)
    ci = S["circuits"][0]
    ci["fixed"][1] = ci["advice"][1]
    g = fresh_graph()
    both = g.add_calculation(q.SUB, (q.FIXED, 1, 0), (q.ADVICE, 1, g.add_rotation(1)))
    g.add_calculation(q.HORNER, (q.PREVIOUS_VALUE, 0, 0), (q.Y, 0, 0), [(q.INTERMEDIATE, 0, 0), both, (q.ADVICE, 2, 0)])
    shared = R.encode(F, ci["advice"][1])
    acc = R.rand(13, n, F)
    arg = R.encode(F, acc) if acc_on == "host" else cuda_off_by_4(R.encode(F, acc))
    got = q.quotient_evaluate_part(
        F.name, n, q.GATES, arg, theta=fr(S["theta"]), beta=fr(S["beta"]), gamma=fr(S["gamma"]), y=fr(S["y"]),
        fixed=[R.encode(F, ci["fixed"][0]), shared],
        advice=[R.encode(F, ci["advice"][0]), shared, cuda_off_by_4(R.encode(F, ci["advice"][2]))],
        instance=[R.encode(F, x) for x in ci["instance"]], challenges=[fr(x) for x in ci["challenges"]], graph=g)
    if acc_on == "cuda":
        assert got is arg
        got = bytes(got.cpu().numpy())
    assert got == want_gates(S, g, acc)


# --- the closed forms ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    cases = [c for c in H.circuits() if c.get("permutations_columns") and H.indicator_polys(c)]
    c = min(cases, key=lambda c: (c["n"], len(c["permutations_columns"])))
    n, omega = c["n"], int(c["omega"], 16)
    sig = [[int(h, 16) for h in col] for col in c["permutations_columns"]]
    cells = G.decode_sigmas(F, sig, omega, G.get_delta(F))
    return n, omega, H.indicator_polys(c)["u"], sig, G.cycle_constant_witness(F, cells, 77)


def gpu_permutation_z(n, u, omega, values, sigmas, beta, gamma, cs_degree, seed):
    """Z columns from the library's grand products, left on the device."""
    import torch
    from tachyon_amd import plonk
    k = (len(values) + cs_degree - 3) // (cs_degree - 2)
    out = [torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(k)]
    blinds = [R.encode(F, R.rand(seed + i, n - u - 1, F)) for i in range(k)]
    res = plonk.permutation_grand_products([values], sigmas, fr(beta), fr(gamma), cs_degree, n, u, fr(omega),
                                           blinds=blinds, out=out)
    assert res is not None
    return out


@pytest.mark.parametrize("L", [1, 2, 7])
def test_permutation(L):
    q = Q()
    n, omega, u, sig, witness = golden()
    cs_degree, delta = L + 2, G.get_delta(F)
    for m in (0, L, L + 1, 2 * L + 1):
        S = R.random_system(F, n, cs_degree, seed=20 + m, perm_m=m, num_lookups=0, num_shuffles=0, u=u)
        S["delta"], ci = delta, S["circuits"][0]
        kinds = ("fixed", "advice", "instance")
        S["perm_columns"], S["sigmas"] = [], [sig[i % len(sig)] for i in range(m)]
        for i in range(m):  # the cycle-constant witness spread over the three kinds
            ci[kinds[i % 3]].append(witness[i % len(witness)])
            S["perm_columns"].append((kinds[i % 3], len(ci[kinds[i % 3]]) - 1))
        values = [R.encode(F, witness[i % len(witness)]) for i in range(m)]
        sigmas = [R.encode(F, x) for x in S["sigmas"]]
        z_dev = gpu_permutation_z(n, u, omega, values, sigmas, S["beta"], S["gamma"], cs_degree, 300) if m else []
        ci["perm_z"] = [R.decode(F, bytes(z.cpu().numpy())) for z in z_dev]
        h = R.rand(40 + m, 1, F)[0]  # the coset's offset: X on row j is h omega^j
        acc = R.rand(41, n, F)
        enc = lambda cols: [R.encode(F, x) for x in cols]
        got = q.quotient_evaluate_part(
            F.name, n, q.PERMUTATION, R.encode(F, acc), cs_degree=cs_degree, last_row=S["last_row"], theta=fr(S["theta"]),
            beta=fr(S["beta"]), gamma=fr(S["gamma"]), y=fr(S["y"]), fixed=enc(ci["fixed"]), advice=enc(ci["advice"]),
            instance=enc(ci["instance"]), challenges=[fr(x) for x in ci["challenges"]], l_first=R.encode(F, S["l_first"]),
            l_last=R.encode(F, S["l_last"]), l_active_row=R.encode(F, S["l_active_row"]), z=z_dev,
            perm_columns=S["perm_columns"], sigmas=sigmas, x_scale=fr(S["beta"] * h % F.p), omega=fr(omega), delta=fr(delta))
        want = R.part(F, S, lambda j: h * pow(omega, j, F.p) % F.p, acc, ("permutation",))
        assert got == R.encode(F, want), m
        if m == 0:
            assert got == R.encode(F, acc)


@pytest.mark.parametrize("count", [0, 1, 2])
def test_lookups_and_shuffles(count):
    """0, 1 or 2 lookups, then as many shuffles (Halo2's indexing: shuffle k reads product k)."""
    q, n = Q(), 2 * T()
    S = R.random_system(F, n, 4, seed=50 + count, perm_m=0, num_lookups=count, num_shuffles=count)
    ci = S["circuits"][0]
    enc = lambda cols: [R.encode(F, x) for x in cols]
    common = dict(cs_degree=4, theta=fr(S["theta"]), beta=fr(S["beta"]), gamma=fr(S["gamma"]), y=fr(S["y"]),
                  fixed=enc(ci["fixed"]), advice=enc(ci["advice"]), instance=enc(ci["instance"]),
                  challenges=[fr(x) for x in ci["challenges"]], l_first=R.encode(F, S["l_first"]),
                  l_last=R.encode(F, S["l_last"]), l_active_row=R.encode(F, S["l_active_row"]))
    acc = R.encode(F, R.rand(51, n, F))
    for k in range(count):
        z, a, s = ci["lookups"][k]
        acc = q.quotient_evaluate_part(F.name, n, q.LOOKUP, acc, graph=R.graph_of(F.name, "lookup", S["lookups"][k]),
                                       z=[R.encode(F, z)], a_perm=R.encode(F, a), s_perm=R.encode(F, s), **common)
        assert acc is not None
    want = R.part(F, S, lambda j: 1, R.rand(51, n, F), ("lookups",))
    assert acc == R.encode(F, want)
    for k in range(count):
        gi, gs = R.graph_of(F.name, "shuffle", S["shuffles"][k])
        acc = q.quotient_evaluate_part(F.name, n, q.SHUFFLE, acc, graph=gi, graph2=gs,
                                       z=[R.encode(F, ci["shuffle_z"][k])], **common)
    assert acc == R.encode(F, R.part(F, S, lambda j: 1, want, ("shuffles",)))


# --- h(X) end to end -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(field_name, n, cs_degree, num_circuits, seed, num_lookups=1, num_shuffles=1):
    field = F if field_name == F.name else FB
    S = R.random_system(field, n, cs_degree, num_circuits=num_circuits, seed=seed, num_lookups=num_lookups,
                        num_shuffles=num_shuffles)
    h, full, w_ext = R.h_poly(field, S)
    return S, R.encode(field, h), R.encode(field, full), w_ext


def call_h(field, S, w_ext=None, conv=None, **extra):
    circuits, kw = R.library_kwargs(field, S, conv)
    return Q().quotient_h_poly(field.name, S["n"], circuits, zeta=fr(S["zeta"], field), delta=fr(S["delta"], field),
                               ext_gen=None if w_ext is None else fr(w_ext, field), **kw, **extra)


@pytest.mark.parametrize("rows", ["16", "T"])
@pytest.mark.parametrize("cs_degree", [3, 4, 5, 9])
def test_h_poly_random_columns(cs_degree, rows):
    n = eval(rows, {"T": T()})
    S, want, want_full, w_ext = reference(F.name, n, cs_degree, 1, 60 + cs_degree)
    assert len(want_full) == 32 * n * {3: 2, 4: 4, 5: 4, 9: 8}[cs_degree]
    assert call_h(F, S, w_ext) == want
    if cs_degree == 4:
        assert call_h(F, S, w_ext, full=True) == want_full and want_full[:len(want)] == want
        assert call_h(F, S, None) == want  # the field's own root: the oracle's default domain


def test_h_poly_two_circuits_and_tensors():
    import torch
    n = T()
    S, want, want_full, w_ext = reference(F.name, n, 4, 2, 70, 2, 2)
    assert call_h(F, S, w_ext) == want
    one, *_ = reference(F.name, n, 4, 1, 70, 2, 2)
    assert call_h(F, one, w_ext) != want  # the second circuit's terms are in
    out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    got = call_h(F, S, w_ext, conv=cuda, out=out)
    assert got is out and bytes(out.cpu().numpy()) == want
    full = torch.zeros(len(want_full), dtype=torch.uint8, device="cuda")
    assert call_h(F, S, w_ext, conv=cuda, out=full, full=True) is full and bytes(full.cpu().numpy()) == want_full
    # no gates, no lookups, no shuffles, no permutation: h = 0
    E = R.random_system(F, 16, 3, seed=71, perm_m=0, num_lookups=0, num_shuffles=0)
    E["gates"] = None
    assert call_h(F, E) == R.encode(F, [0] * 32)
    E["gates"], E["empty_gates"] = [], True
    assert call_h(F, E) == R.encode(F, [0] * 32)


def test_h_poly_bls12_381():
    S, want, _, w_ext = reference(FB.name, 64, 4, 1, 80)
    assert call_h(FB, S, w_ext) == want
    assert call_h(FB, S, None) == want


@pytest.mark.parametrize("cs_degree", [4, 6])
def test_h_poly_satisfied_circuit(cs_degree):
    """Gate s (a b - c), a real permutation Z over a golden sigma set (from
    the library's grand products), a sorted one-column lookup and a shuffle:
    bytewise, the identity at two points, and no coefficient from
    n (cs_degree - 1) up."""
    n, omega, u, sig, witness = golden()
    with O.halo2_domain():
        probe = R.satisfied_system(F, n, u, omega, sig, witness, cs_degree)
        z_dev = gpu_permutation_z(n, u, omega, [R.encode(F, w) for w in witness], [R.encode(F, x) for x in sig],
                                  probe["beta"], probe["gamma"], cs_degree, 900)
        S = R.satisfied_system(F, n, u, omega, sig, witness, cs_degree,
                               perm_z_evals=[R.decode(F, bytes(z.cpu().numpy())) for z in z_dev])
        h, full, w_ext = R.h_poly(F, S)
    assert pow(w_ext, len(full) // n, F.p) == omega
    got = call_h(F, S, w_ext, full=True)
    assert got == R.encode(F, full)
    coeffs = R.decode(F, got)
    assert any(coeffs) and not any(coeffs[n * (cs_degree - 1):])
    assert call_h(F, S, w_ext) == R.encode(F, h)
    for x in R.rand(33, 2, F):
        assert R.identity_at(F, S, omega, coeffs[:n * (cs_degree - 1)], x)


@pytest.mark.parametrize("shape", [(64, 4, 1), (256, 9, 2)])
def test_work_bytes_covers_the_call(shape):
    n, cs_degree, num_circuits = shape
    S, want, _, w_ext = reference(F.name, n, cs_degree, num_circuits, 90)
    circuits, kw = R.library_kwargs(F, S)
    est = Q().quotient_work_bytes(F.name, n, circuits, **kw)
    assert call_h(F, S, w_ext) == want
    held = Q().held_bytes()
    print(f"MEM n={n} cs_degree={cs_degree} circuits={num_circuits} work_bytes={est} held_bytes={held}")
    polys = len({id(p) for p in R.all_polys(S)})
    N = n << (R.extended_k(n, cs_degree) - (n.bit_length() - 1))
    assert held >= 32 * (polys * n + N + n)  # the cosets, the extended buffer, the accumulator
    assert 0 < held <= est <= 3 * held


# --- refusals ------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    import torch
    q, n = Q(), 16
    S, want, _, w_ext = reference(F.name, n, 4, 1, 64)
    out = torch.full((len(want),), 0xA5, dtype=torch.uint8, device="cuda")
    untouched = bytes(out.cpu().numpy())

    def refused(damage, **extra):
        B = dict(S)
        B["circuits"] = [dict(c) for c in S["circuits"]]
        damage(B)
        return call_h(F, B, w_ext, out=out, **extra) is None and bytes(out.cpu().numpy()) == untouched

    low = dict(S, cs_degree=2)  # n (cs_degree - 1) coefficients would be another size: host bytes out
    assert call_h(F, low, w_ext) is None
    assert refused(lambda B: B.update(perm_columns=[("advice", 3)] + B["perm_columns"][1:]))  # names no column
    assert refused(lambda B: B["circuits"][0].update(perm_z=B["circuits"][0]["perm_z"][:1]))  # z count
    assert refused(lambda B: B.update(gates=[("advice", 9, 0)]))  # column index
    assert refused(lambda B: B.update(lookups=[([("challenge", 1)], [("fixed", 0, 0)])]))  # challenge index
    assert refused(lambda B: B.update(gates=[("fixed", 2, 0)]))
    # an extended generator of another order: refused after validation, with a message, nothing written
    assert call_h(F, S, pow(w_ext, 2, F.p), out=out) is None and bytes(out.cpu().numpy()) == untouched
    assert call_h(F, S, w_ext, out=out) is out and bytes(out.cpu().numpy()) == want

    # hand-damaged graphs through evaluate_part: the accumulator stays as it was
    T0 = table_system(n, seed=7)
    acc = R.rand(13, n, F)
    ok = fresh_graph()
    ok.add_calculation(q.ADD, (q.INTERMEDIATE, 0, 0), (q.BETA, 0, 0))
    assert run_gates(T0, ok, acc) is not None
    cases = {
        "kind": lambda g: g.add_calculation(q.ADD, (11, 0, 0), (q.BETA, 0, 0)),
        "op": lambda g: g.add_calculation(8, (q.BETA, 0, 0), (q.BETA, 0, 0)),
        "constant": lambda g: g.add_calculation(q.ADD, (q.CONSTANT, 4, 0), (q.BETA, 0, 0)),
        "rotation": lambda g: g.add_calculation(q.STORE, (q.ADVICE, 0, 1)),
        "instance": lambda g: g.add_calculation(q.STORE, (q.INSTANCE, 1, 0)),
        "challenge": lambda g: g.add_calculation(q.STORE, (q.CHALLENGE, 1, 0)),
        "read before write": lambda g: g.add_calculation(q.DOUBLE, (q.INTERMEDIATE, 1, 0)),
        "horner part": lambda g: g.add_calculation(q.HORNER, (q.BETA, 0, 0), (q.Y, 0, 0), [(q.FIXED, 2, 0)]),
    }
    for name, damage in cases.items():
        g = fresh_graph()
        damage(g)
        dev = cuda(R.encode(F, acc))
        before = bytes(dev.cpu().numpy())
        ci = T0["circuits"][0]
        enc = lambda cols: [R.encode(F, x) for x in cols]
        res = q.quotient_evaluate_part(F.name, n, q.GATES, dev, theta=fr(1), beta=fr(2), gamma=fr(3), y=fr(4),
                                       fixed=enc(ci["fixed"]), advice=enc(ci["advice"]), instance=enc(ci["instance"]),
                                       challenges=[fr(5)], graph=g)
        assert res is None and bytes(dev.cpu().numpy()) == before, name
    for bad_n in (0, 1, 12):
        with pytest.raises(ValueError):
            run_gates(dict(T0, n=bad_n), ok, acc)  # the wrapper's own size check
    # n that is no power of two, with columns of that length
    T12 = table_system(16, seed=8)
    T12["n"] = 12
    T12["circuits"] = [{k: ([x[:12] for x in v] if k != "challenges" else v) for k, v in T12["circuits"][0].items()}]
    assert run_gates(T12, ok, acc[:12]) is None


# --- the permutation's label past one workgroup -----------------------------------------
def permutation_part(S, n, h, omega, acc, enc):
    """quotient_evaluate_part(PERMUTATION) on circuit 0 of S, X on row j = h omega^j;
    enc(column) gives the bytes of a column of S."""
    q, ci = Q(), S["circuits"][0]
    cols = lambda xs: [enc(x) for x in xs]
    return q.quotient_evaluate_part(
        F.name, n, q.PERMUTATION, acc, cs_degree=S["cs_degree"], last_row=S["last_row"], theta=fr(S["theta"]),
        beta=fr(S["beta"]), gamma=fr(S["gamma"]), y=fr(S["y"]), fixed=cols(ci["fixed"]), advice=cols(ci["advice"]),
        instance=cols(ci["instance"]), challenges=[fr(x) for x in ci["challenges"]], l_first=enc(S["l_first"]),
        l_last=enc(S["l_last"]), l_active_row=enc(S["l_active_row"]), z=cols(ci["perm_z"]),
        perm_columns=S["perm_columns"], sigmas=cols(S["sigmas"]), x_scale=fr(S["beta"] * h % F.p), omega=fr(omega),
        delta=fr(S["delta"]))


def test_permutation_label_on_a_second_workgroup():
    """n = 2T: the label x_scale omega^row of rows T .. 2T-1 takes the second
    entry of the per-tile power table; every row compared."""
    n = 2 * T()
    S = R.random_system(F, n, 4, seed=23, perm_m=5, num_lookups=0, num_shuffles=0)
    omega, h = F.root_of_unity(1 << 24), R.rand(24, 1, F)[0]
    acc = R.rand(25, n, F)
    got = permutation_part(S, n, h, omega, R.encode(F, acc), lambda x: R.encode(F, x))
    want = R.part(F, S, lambda j: h * pow(omega, j, F.p) % F.p, acc, ("permutation",))
    assert got == R.encode(F, want)


def test_permutation_label_past_65536_rows():
    """n = 2^17: rows from 65536 on read the third power table's second entry
    and rows 65280 .. 65535 the second table's last; the reference is computed
    on sampled rows -- a tile's first and last, both sides of 65536, the end."""
    n, t = 1 << 17, T()
    S = R.random_system(F, 16, 4, seed=26, perm_m=3, num_lookups=0, num_shuffles=0)
    S["n"], S["last_row"] = n, -5
    seeds = iter(range(2600, 2700))
    column = lambda _=None: O.gen_scalars(F.name, next(seeds), n).tobytes()
    for key in ("l_first", "l_last", "l_active_row"):
        S[key] = column()
    S["sigmas"] = [column() for _ in S["sigmas"]]
    ci = S["circuits"][0]
    for key in ("fixed", "advice", "instance", "perm_z"):
        ci[key] = [column() for _ in ci[key]]
    omega, h = F.root_of_unity(1 << 24), R.rand(27, 1, F)[0]
    acc = column()
    got = permutation_part(S, n, h, omega, acc, lambda b: b)
    assert got is not None
    at = lambda col, j: F.from_bytes(col[32 * j:32 * j + 32])
    for j in (0, 1, t - 1, t, 2 * t - 1, 65535 - t, 65535, 65536, 65536 + t, 65536 + 255 * t, n - t, n - 1):
        want = R.numerator(F, S, lambda col, rot, j=j: at(col, (j + rot) % n), h * pow(omega, j, F.p) % F.p,
                           at(acc, j), ("permutation",))
        assert at(got, j) == want, j


# --- refusals that only the library can decide ---------------------------------------------
class DamagedGraph:
    """A GraphEvaluator whose C image is altered after it is filled: what the
    Python builder cannot express (a target or a Horner range out of bounds)."""

    def __init__(self, graph, damage):
        self.graph, self.damage = graph, damage

    def fill(self, dst, keep):
        self.graph.fill(dst, keep)
        self.damage(dst)


def test_refusals_decided_by_the_library():
    import ctypes
    import torch
    from tachyon_amd._lib import lib
    q, n = Q(), 16
    S = table_system(n, seed=7)
    ci = S["circuits"][0]
    enc = lambda cols: [R.encode(F, x) for x in cols]
    col = R.encode(F, ci["advice"][0])
    acc = cuda(R.encode(F, R.rand(13, n, F)))
    before = bytes(acc.cpu().numpy())
    base = dict(theta=fr(1), beta=fr(2), gamma=fr(3), y=fr(4), fixed=enc(ci["fixed"]), advice=enc(ci["advice"]),
                instance=enc(ci["instance"]), challenges=[fr(5)])
    good = fresh_graph()
    good.add_calculation(q.HORNER, (q.PREVIOUS_VALUE, 0, 0), (q.Y, 0, 0), [(q.INTERMEDIATE, 0, 0), (q.BETA, 0, 0)])
    lookup = R.graph_of(F.name, "lookup", R.LOOKUP_EXPRS)
    closed = dict(base, cs_degree=4, l_first=col, l_last=col, l_active_row=col)

    def set_calc(field, value, index=-1):
        def damage(dst):
            setattr(dst.calcs[dst.num_calcs + index if index < 0 else index], field, value)
        return damage

    cases = {
        "null theta": (q.GATES, dict(base, theta=None, graph=good)),
        "null y": (q.GATES, dict(base, y=None, graph=good)),
        "null graph": (q.GATES, dict(base, graph=None)),
        "lookup without l_first": (q.LOOKUP, dict(closed, l_first=None, graph=lookup, z=[col], a_perm=col, s_perm=col)),
        "lookup without a_perm": (q.LOOKUP, dict(closed, graph=lookup, z=[col], a_perm=None, s_perm=col)),
        "lookup without z": (q.LOOKUP, dict(closed, graph=lookup, z=[], a_perm=col, s_perm=col)),
        "shuffle without its second graph": (q.SHUFFLE, dict(closed, graph=lookup, graph2=None, z=[col])),
        "group kind": (4, dict(base, graph=good)),
        "target >= num_intermediates": (q.GATES, dict(base, graph=DamagedGraph(good, set_calc("target", 2)))),
        "num_intermediates below a target": (q.GATES, dict(base, graph=DamagedGraph(
            good, lambda dst: setattr(dst, "num_intermediates", 1)))),
        "Horner parts past the end": (q.GATES, dict(base, graph=DamagedGraph(good, set_calc("parts_count", 3)))),
        "Horner parts begin past the end": (q.GATES, dict(base, graph=DamagedGraph(good, set_calc("parts_begin", 3)))),
        "null calcs": (q.GATES, dict(base, graph=DamagedGraph(good, lambda dst: setattr(dst, "calcs", None)))),
        "null constants": (q.GATES, dict(base, graph=DamagedGraph(good, lambda dst: setattr(dst, "constants", None)))),
    }
    assert q.quotient_evaluate_part(F.name, n, q.GATES, acc.clone(), graph=good, **base) is not None
    for name, (kind, kw) in cases.items():
        assert q.quotient_evaluate_part(F.name, n, kind, acc, **kw) is None, name
        assert bytes(acc.cpu().numpy()) == before, name
    # n < 2, with columns of exactly n elements so that the call reaches the library
    for bad_n in (0, 1):
        short = dict(base, fixed=[col[:32 * bad_n]] * 2, advice=[col[:32 * bad_n]] * 3, instance=[col[:32 * bad_n]])
        assert q.quotient_evaluate_part(F.name, bad_n, q.GATES, col[:32 * bad_n], graph=good, **short) is None

    # log2(n P) above the field's two-adicity: only the descriptors are read,
    # so one element stands for every polynomial (the wrapper would ask for n)
    elem = ctypes.create_string_buffer(fr(7), 32)
    ptr = ctypes.cast(elem, ctypes.c_void_p)
    params = q.QParams()
    params.field, params.cs_degree = 0, 4
    for name in ("theta", "beta", "gamma", "y", "l_first", "l_last", "l_active_row"):
        setattr(params, name, ptr)
    system, circuit = q.QSystem(), (q.QCircuit * 1)()
    out = ctypes.create_string_buffer(b"\xA5" * 64, 64)
    L = lib()
    params.n = 1 << 26  # extended_k = 28: the field's two-adicity
    assert L.tachyon_mi355x_quotient_work_bytes(ctypes.byref(params), ctypes.byref(system), circuit, 1) > 0
    params.n = 1 << 27
    assert L.tachyon_mi355x_quotient_work_bytes(ctypes.byref(params), ctypes.byref(system), circuit, 1) == 0
    assert L.tachyon_mi355x_quotient_h_poly(ctypes.byref(params), ctypes.byref(system), circuit, 1, ptr, ptr, None, 0,
                                            out) == 0
    params.n = 16
    for args in ((None, ctypes.byref(system), circuit, 1, ptr, ptr, None, 0, out),
                 (ctypes.byref(params), None, circuit, 1, ptr, ptr, None, 0, out),
                 (ctypes.byref(params), ctypes.byref(system), None, 1, ptr, ptr, None, 0, out),
                 (ctypes.byref(params), ctypes.byref(system), circuit, 1, None, ptr, None, 0, out),
                 (ctypes.byref(params), ctypes.byref(system), circuit, 1, ptr, ptr, None, 0, None)):
        assert L.tachyon_mi355x_quotient_h_poly(*args) == 0
    assert out.raw == b"\xA5" * 64

    # a zeta whose coset meets the domain: X^n - 1 has no inverse on a part
    Sr, want, _, w_ext = reference(F.name, 16, 4, 1, 64)
    dev = torch.full((len(want),), 0xA5, dtype=torch.uint8, device="cuda")
    assert call_h(F, dict(Sr, zeta=1), w_ext, out=dev) is None
    assert bytes(dev.cpu().numpy()) == b"\xA5" * len(want)
