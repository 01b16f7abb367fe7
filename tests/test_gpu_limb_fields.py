"""The carry-free limb fields on the device at their operand bounds: the code
the hot kernels run -- the generated v_mad_u64_u32 products of field/f29_asm.h,
f28_asm.h and fr29_gen.h, the device's float quotient, the point formulas of
msm/acc29.h and acc28.h and, alone for the first time, the lane-pair G2
formulas of msm/pair29.h and pair28.h -- through tachyon_mi355x_limb_op on raw
limbs, against the shared exact model (tests/limb_model.py, pinned to the host
build by tests/test_limb_model.py).

Limb-exact (Python integers, zero tolerance): every product (mul, mul_add,
mul2_add with four and five operands, sqr, sqr_add, pmul / pmul_add / psqr /
psqr_add for every constant the formulas use, fr29 mont and shoup), normalize,
to32, from_words, to_canonical_words, is_zero_mod_p / pzero, and the point
formulas that contain no float quotient (acc29 / acc28 madd, add, dbl; pair28
madd, add, dbl).  Contract only (residue mod p, N-form, the documented bound):
reduce_shl5 / reduce, from32, from_shifted, the fr29 register steps and the
pair29 formulas, which call reduce_shl5 -- its quotient may be q* - 2 .. q*,
and the rounding of the float multiply belongs to the compiler."""
import ctypes
import random

import numpy as np
import pytest

import limb_model as L
from limb_model import F28, F29, FR29, PAIR28, PAIR29

pytestmark = pytest.mark.gpu

FAMILY = {"f29": 0, "f28": 1, "fr29": 2}
FQ = [F29, F28]
OPS = {"mul": 0, "mul_add": 1, "mul2_add": 2, "mul2_add5": 3, "sqr": 4, "sqr_add": 5, "normalize": 6, "from32": 7,
       "to32": 8, "is_zero": 9, "reduce": 10, "start": 11, "madd": 12, "add": 13, "dbl": 14,
       "pzero": 20, "pstart": 21, "pmadd": 22, "padd": 23, "pdbl": 24}
FR_OPS = {"mont": 0, "shoup": 1, "reduce": 2, "from_words": 3, "canon": 4, "radix4s": 5, "radix4m": 6,
          "radix4last": 7, "radix2": 8, "radix2last": 9}
ids = lambda F: F.name  # noqa: E731


def device(F, op, rows):
    """rows of flat operand words through the device op; rows of result words"""
    from tachyon_amd._lib import lib
    fam = FAMILY[F.name]
    iw, ow = ctypes.c_int(), ctypes.c_int()
    assert lib().tachyon_mi355x_limb_op_words(fam, op, ctypes.byref(iw), ctypes.byref(ow)), (F.name, op)
    a = np.array(rows, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[1] == iw.value and int(a.max()) < (1 << 32), (a.shape, iw.value)
    a = np.ascontiguousarray(a.astype(np.uint32))
    out = np.zeros((a.shape[0], ow.value), dtype=np.uint32)
    lib().tachyon_mi355x_limb_op(fam, op, a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                                 a.shape[0])
    return out.tolist()


def flat(*xs):
    return [t for x in xs for t in x]


def pflat(*pairs):
    """lane-pair values (c0 limbs, c1 limbs) as the device lays them out"""
    return [t for c0, c1 in pairs for t in c0 + c1]


def chunks(v, k):
    return [v[i:i + k] for i in range(0, len(v), k)]


# ---------------------------------------------------------------- products
@pytest.mark.parametrize("F", FQ, ids=ids)
def test_products_limb_exact(F):
    """Every single-lane product on the operands of its call sites (the
    limb-wise ksub / add_ksub / ksub2 / times results of top-of-bound values,
    the squares' a0 + a1 and a0 + K - a1), random values over the same ranges,
    all-ones low limbs, zero, forced Montgomery digits 0 and 2^W - 1 and
    addends carrying into the top limb: the device limbs equal the integer
    formula's."""
    rng = random.Random(101)
    cases = L.product_cases(F, rng, 250)
    got = {}
    for op, lst in cases.items():
        got[op] = device(F, OPS[op], [flat(*ops) for ops in lst])
        want = [L.product_expected(F, op, ops) for ops in lst]
        bad = [i for i, (g, w) in enumerate(zip(got[op], want)) if g != w]
        print(f"{F.name} {op}: {len(lst)} cases, {len(bad)} mismatches")
        assert not bad, (op, len(bad), lst[bad[0]], got[op][bad[0]], want[bad[0]])
    # the dedicated squares against the general products on the same operands
    assert got["sqr"] == device(F, OPS["mul"], [flat(a, a) for a, in cases["sqr"]])
    assert got["sqr_add"] == device(F, OPS["mul_add"], [flat(a, a, e) for a, e in cases["sqr_add"]])


@pytest.mark.parametrize("PM", [PAIR29, PAIR28], ids=lambda PM: PM.F.name)
def test_pair_products_limb_exact(PM):
    """pmul / pmul_add / psqr / psqr_add for every constant K that madd, add
    and dbl instantiate them with, both lanes, on the operands of those call
    sites: limb-exact against the model's two lanes."""
    F = PM.F
    rng = random.Random(102)
    for (kind, Kn), lst in L.pair_product_cases(PM, rng, 400).items():
        op = 32 + 8 * L.PAIR_KINDS[kind] + L.PAIR_K[Kn]
        rows = [pflat(*[x for x in case if x is not None]) for case in lst]
        got = device(F, op, rows)
        bad = 0
        for (a, b, e), g in zip(lst, got):
            w0, w1 = L.pair_product_expected(PM, kind, Kn, a, b, e)
            bad += g != w0 + w1
        print(f"{F.name} {kind}<{Kn}>: {len(lst)} cases, {bad} mismatches")
        assert bad == 0, (kind, Kn)


def test_fr29_products_limb_exact():
    """mont and shoup on the butterflies' operands (limbs up to 2^31.3: the
    worst-case stage inputs of test_fr29_host.max_inputs, random wide limbs)
    with twiddles 0, 1, p - 1, p - 2 and random: the device limbs equal the
    column model's, mont also the integer formula's."""
    from test_fr29_host import max_inputs, mont_tw, shoup_tw
    G = L.gen_fr29
    rng = random.Random(103)
    amax = max_inputs()
    cases = []
    for t in range(3000):
        w = rng.randrange(FR29.P) if t % 5 else rng.choice([0, 1, FR29.P - 1, FR29.P - 2])
        a = amax[t % 3] if t % 4 == 0 else [rng.randrange(1 << 31) for _ in range(8)] + [rng.randrange(1 << 26)]
        cases.append((a, w))
    gm = device(FR29, FR_OPS["mont"], [flat(a, mont_tw(w)) for a, w in cases])
    gs = device(FR29, FR_OPS["shoup"], [flat(a, *shoup_tw(w)) for a, w in cases])
    for (a, w), rm, rs in zip(cases, gm, gs):
        assert rm == G.mont(a, mont_tw(w))[0] == FR29.product_case(a, mont_tw(w)), (a, w)
        assert rs == G.shoup(a, *shoup_tw(w))[0], (a, w)
        assert FR29.value(rs) % FR29.P == FR29.value(a) * w % FR29.P


# ------------------------------------------- conversions, the float quotient
def _words_near(F, v):
    """R-form words x~ whose shifted value x~ << SHIFT is the nearest at or above v"""
    return -(-v >> F.SHIFT)


@pytest.mark.parametrize("F", FQ, ids=ids)
def test_reduce_and_conversions(F):
    """reduce_shl5 / reduce and from32 over their whole input range, at every
    quotient boundary q p + d and at float32 rounding midpoints of the top two
    limbs: the contract (residue, N-form, < 3p, quotient q* - 2 .. q*).
    to32 and normalize are integer-only: exact."""
    rng = random.Random(104)
    p, s = F.P, F.SHIFT
    vmax, every = L.REDUCE_RANGE[F.name]
    inputs = L.reduce_inputs(F, rng, vmax, every, n_random=2000)
    for v, r in zip(inputs, device(F, OPS["reduce"], inputs)):
        L.check_reduced(F, v, r)
    # from32: words x~ < 2^255 (f29), lazy < 2p (f28)
    xmax = (1 << 255) if F.name == "f29" else 2 * p
    xs = [0, 1, p - 1, p, min(2 * p, xmax) - 1, xmax - 1] + [rng.randrange(xmax) for _ in range(1000)]
    for q in range((xmax << s) // p + 1):
        xs += [_words_near(F, q * p) - 1, _words_near(F, q * p), _words_near(F, q * p + 1)]
    xs += [F.value(v) >> s for v in inputs[-300:]]  # the rounding midpoints (their low bits dropped)
    xs = [x for x in xs if 0 <= x < xmax]
    got = device(F, OPS["from32"], [F.words(x) for x in xs])
    for x, r in zip(xs, got):
        L.check_reduced(F, F.limbs(x << s), r)
    print(f"{F.name}: reduce {len(inputs)} inputs, from32 {len(xs)}")
    # to32: N-form below 16p -> (x + k p) / 2^SHIFT exactly, k the Montgomery digit; below 2p
    ys = [0, 1, p, 16 * p - 1, F.value(L.ones(F, 16))] + [k * p + d for k in range(16) for d in (0, 1, p - 1)]
    ys += [rng.randrange(16 * p) for _ in range(1500)]
    ys += [F.value(F.limbs(y)[:1] + [F.M] * (F.N - 2) + F.limbs(y)[-1:]) for y in ys[:200]]
    ys = [y for y in ys if y < 16 * p]
    for y, w in zip(ys, device(F, OPS["to32"], [F.limbs(y) for y in ys])):
        k = (-y * pow(p, -1, 1 << s)) % (1 << s)
        v = sum(t << (32 * i) for i, t in enumerate(w))
        assert v == (y + k * p) >> s and v < 2 * p and v % p == y * pow(2, -s, p) % p, y
    # normalize: limb-wise sums and multiples, up to the widest limbs a 32-bit register carries
    # through (limb + carry < 2^32 with a carry below 2^(32 - W): limbs up to 2^32 - 2^(32 - W))
    zs = [F.times(L.ones(F, 10), 3), F.times(L.ones(F, 3), 2), F.add(L.ones(F, 10), F.K["K16"]), [0] * F.N]
    wide = (1 << 32) - (1 << (32 - F.W)) + 1
    zs += [[rng.randrange(wide) for _ in range(F.N - 1)] + [rng.randrange(1 << 31)] for _ in range(1000)]
    zs += [[wide - 1] * (F.N - 1) + [(1 << 31)]]
    for z, r in zip(zs, device(F, OPS["normalize"], zs)):
        assert r == F.normalize(z) and F.value(r) == F.value(z) and F.n_form(r), z


def test_fr29_reduce_and_words():
    """fr29::reduce over values below 2^264 with limbs up to 2^32 (every
    quotient boundary, rounding midpoints, unnormalized limbs): the contract;
    from_words and to_canonical_words: exact."""
    F = FR29
    rng = random.Random(105)
    vmax, every = L.REDUCE_RANGE["fr29"]
    inputs = L.reduce_inputs(F, rng, vmax, every)
    wide = [[rng.randrange(1 << 32) for _ in range(9)] for _ in range(500)] + [[(1 << 32) - 1] * 9]
    got = device(F, FR_OPS["reduce"], inputs + wide)
    for v, r in zip(inputs, got):
        L.check_reduced(F, v, r)
    for v, r in zip(wide, got[len(inputs):]):  # unnormalized: the value counts
        assert F.value(r) % F.P == F.value(v) % F.P and F.value(r) < 3 * F.P and F.n_form(r), v
    canon = inputs + wide
    for v, w in zip(canon, device(F, FR_OPS["canon"], canon)):
        assert sum(t << (32 * i) for i, t in enumerate(w)) == F.value(v) % F.P, v
    ws = [[rng.randrange(1 << 32) for _ in range(8)] for _ in range(500)] + [[0xFFFFFFFF] * 8, [0] * 8]
    for w, r in zip(ws, device(F, FR_OPS["from_words"], ws)):
        assert F.value(r) == sum(t << (32 * i) for i, t in enumerate(w)) and F.n_form(r)
    print(f"fr29: reduce {len(inputs) + len(wide)}, canon {len(canon)}, from_words {len(ws)}")


# ------------------------------------------------------------- zero tests
@pytest.mark.parametrize("F", FQ, ids=ids)
def test_is_zero_and_pzero(F):
    """k p and k p +- 1 for every k of the documented range, random values,
    and k p + j 2^32: the one-multiply filter passes them (the low word is
    k p's) and the full limb compare must refuse them.  pzero: both lanes
    report the AND, with only one component zero as well."""
    rng = random.Random(106)
    p, kmax = F.P, F.ZERO_K
    xs = [k * p + d for k in range(kmax) for d in (0, 1, -1) if k * p + d >= 0]
    xs += [rng.randrange(kmax * p) for _ in range(1000)]
    filt = [k * p + (j << 32) for k in range(kmax) for j in
            [1, 2, 1 << (F.W - 3)] + [rng.randrange(1, p >> 40) for _ in range(20)]]
    for x in filt:  # they do pass the filter
        assert ((x & 0xFFFFFFFF) * F.PINV32) & 0xFFFFFFFF < kmax and x % p and x < kmax * p
    xs += filt
    got = device(F, OPS["is_zero"], [F.limbs(x) for x in xs])
    bad = [x for x, r in zip(xs, got) if r[0] != int(x % p == 0)]
    assert not bad, (len(bad), bad[0])
    zeros = [k * p for k in range(kmax)]
    pairs = []
    for _ in range(600):
        c = [rng.choice(zeros) if rng.random() < 0.6 else rng.choice(filt + xs) for _ in range(2)]
        pairs.append(tuple(c))
    for (c0, c1), r in zip(pairs, device(F, OPS["pzero"], [pflat((F.limbs(c0), F.limbs(c1))) for c0, c1 in pairs])):
        assert r == [int(c0 % p == 0 and c1 % p == 0)] * 2, (c0, c1)
    print(f"{F.name}: is_zero {len(xs)} ({len(filt)} filter-passing), pzero {len(pairs)}")


# --------------------------------------------------- single-lane formulas
@pytest.mark.parametrize("F", FQ, ids=ids)
def test_point_formulas_at_bounds(F):
    """The cases of the host test_point_formulas_at_bounds through the device
    code: the affine result, `special`, N-form limbs, the invariant's output
    bounds, and -- madd, add and dbl contain no float quotient -- the limbs of
    the model's formulas."""
    rng = random.Random(107)
    N, p = F.N, F.P
    cases = L.point_cases(F, rng, 24)
    by_op = {}
    for c in cases:
        by_op.setdefault(c[0], []).append(c)
    model = {"madd": lambda v: L.acc_madd(F, v[:4], v[4], v[5]), "add": lambda v: L.acc_add(F, v[:4], v[4:]),
             "dbl": lambda v: (0, L.acc_dbl(F, v))}
    for op, lst in by_op.items():
        got = device(F, OPS[op], [c[1] for c in lst])
        for (_, operands, expect, special), g in zip(lst, got):
            sp, pt, vals, v = F.point_of([g[4 * N]] + g[:4 * N])
            assert sp == special, (op, sp, special)
            if op != "start":
                msp, macc = model[op](chunks(operands, N))
                assert msp == special and g[:4 * N] == flat(*macc), op  # specials: acc unchanged
            if special:
                continue
            assert pt == expect, op
            X, Y, ZZ, ZZZ = vals
            assert X < 10 * p and Y < 3 * p and ZZ < 3 * p and ZZZ < 3 * p, op
            assert all(F.n_form(c) for c in chunks(v, N)), op
        print(f"{F.name} {op}: {len(lst)} cases")


# ------------------------------------------------------- lane-pair formulas
def _pair_out(F, g):
    N = F.N
    vals = chunks(g[:8 * N], N)
    return tuple((vals[2 * i], vals[2 * i + 1]) for i in range(4)), g[8 * N:]


def _scaled(PM, rng, A, bounds):
    """another representative of the point of A: (X l^2, Y l^3, ZZ l^2, ZZZ l^3)"""
    F = PM.F
    lam = (rng.randrange(1, F.P), rng.randrange(F.P))
    l2 = PM.fm(lam, lam)
    l3 = PM.fm(l2, lam)
    vals = [PM.fm(PM.f2(c), s) for c, s in zip(A, (l2, l3, l2, l3))]
    return tuple((F.top_rep(c[0] * F.R1 % F.P, b), F.top_rep(c[1] * F.R1 % F.P, b)) for c, b in zip(vals, bounds))


@pytest.mark.parametrize("PM", [PAIR29, PAIR28], ids=lambda PM: PM.F.name)
def test_pair_point_formulas(PM):
    """The cases of test_pair29_model.py / test_pair28_model.py through the
    real lane-pair code: madd and dbl with the accumulator at the top of its
    input invariant, a run start followed by madd, the specials (both lanes
    agree, the accumulator comes back unchanged), add at the bounds and on
    two representatives of one point.  Fq2 coordinates mod p against the
    reference formulas, limb shapes, output bounds; pair28's madd, add and
    dbl hold no float quotient and match the model limb for limb."""
    F = PM.F
    rng = random.Random(108)
    f2 = PM.f2
    exact = F.name == "f28"
    lazy = (lambda: rng.random() < 0.5) if exact else (lambda: False)
    base = lambda x=None: L.pair_base(F, rng, x, lazy=lazy())  # noqa: E731

    # madd and dbl at the bounds
    A_ = [PM.rand_acc(rng) for _ in range(60)]
    B_ = [(base(), base()) for _ in A_]
    got = device(F, OPS["pmadd"], [pflat(*A, x[0], y[0]) for A, (x, y) in zip(A_, B_)])
    for A, ((x2, xv), (y2, yv)), g in zip(A_, B_, got):
        out, sp = _pair_out(F, g)
        assert sp == [0, 0]
        PM.check_out(out, PM.madd_ref(tuple(f2(c) for c in A), xv, yv))
        if exact:
            assert (0, out) == PM.madd(A, x2, y2)
    # the doubling also with Y (and X) on quotient boundaries k p + d of the reduction in front of it
    D_ = list(A_)
    for k in range(PM.IN_BOUNDS[1]):
        A = PM.rand_acc(rng)
        yb = tuple(F.limbs(k * F.P + d) for d in ((0, 1) if k else (1, 2)))
        D_.append((A[0], yb, A[2], A[3]))
    for A, g in zip(D_, device(F, OPS["pdbl"], [pflat(*A) for A in D_])):
        out, _ = _pair_out(F, g)
        PM.check_out(out, PM.dbl_ref(tuple(f2(c) for c in A)))
        if exact:
            assert out == PM.dbl(A)
    # a run's first point, then the next madd on what the device left
    S_ = [(base(), base()) for _ in range(40)]
    started = device(F, OPS["pstart"], [pflat(x[0], y[0]) for x, y in S_])
    N_ = [(base(), base()) for _ in S_]
    rows = []
    for ((x2, xv), (y2, yv)), g in zip(S_, started):
        acc, _ = _pair_out(F, g)
        assert tuple(f2(c) for c in acc) == (xv, yv, (1, 0), (1, 0))
        PM.check_out(acc, (xv, yv, (1, 0), (1, 0)), bounds=PM.IN_BOUNDS if not exact else (3, 3, 3, 3))
        rows.append(acc)
    got = device(F, OPS["pmadd"], [pflat(*acc, x[0], y[0]) for acc, (x, y) in zip(rows, N_)])
    for ((_, xv), (_, yv)), ((_, bxv), (_, byv)), g in zip(S_, N_, got):
        out, sp = _pair_out(F, g)
        assert sp == [0, 0]
        PM.check_out(out, PM.madd_ref((xv, yv, (1, 0), (1, 0)), bxv, byv))
    # the specials: base = the accumulator's point (2: the caller doubles), its negative (1: identity)
    rows, want = [], []
    for _ in range(20):
        A = PM.rand_acc(rng)
        Af = tuple(f2(c) for c in A)
        xv, yv = PM.fm(Af[0], PM.finv(Af[2])), PM.fm(Af[1], PM.finv(Af[3]))
        (x2, _), (y2, _) = base(xv), base(yv)
        (y2n, _) = base(((-yv[0]) % F.P, (-yv[1]) % F.P))
        # only one component of P zero is no special case: x differs in c1 alone
        (x2o, xo) = base((xv[0], (xv[1] + 1) % F.P))
        rows += [pflat(*A, x2, y2), pflat(*A, x2, y2n), pflat(*A, x2o, y2)]
        want += [(2, A, None), (1, A, None), (0, A, (xo, yv))]
    for (special, A, b), g in zip(want, device(F, OPS["pmadd"], rows)):
        out, sp = _pair_out(F, g)
        assert sp == [special, special]
        if special:
            assert out == A
        else:
            PM.check_out(out, PM.madd_ref(tuple(f2(c) for c in A), *b))
    # add at the bounds, and on two representatives of one point / of its negative
    P_ = [(PM.rand_acc(rng, PM.OUT_BOUNDS), PM.rand_acc(rng, PM.OUT_BOUNDS)) for _ in range(60)]
    want = [0] * len(P_)
    for _ in range(10):
        A = PM.rand_acc(rng, PM.OUT_BOUNDS)
        Bs = _scaled(PM, rng, A, PM.OUT_BOUNDS)
        negy = tuple(F.top_rep((-F.value(c)) % F.P, PM.OUT_BOUNDS[1]) for c in Bs[1])
        P_ += [(A, Bs), (A, (Bs[0], negy, Bs[2], Bs[3]))]
        want += [2, 1]
    for (A, B), special, g in zip(P_, want, device(F, OPS["padd"], [pflat(*A, *B) for A, B in P_])):
        out, sp = _pair_out(F, g)
        assert sp == [special, special]
        if special:
            assert out == A
            continue
        PM.check_out(out, PM.add_ref(tuple(f2(c) for c in A), tuple(f2(c) for c in B)))
        if exact:
            assert (0, out) == PM.point_add(A, B)
    print(f"{F.name}: pmadd {len(A_) + len(S_) + len(rows)}, pdbl {len(D_)}, pstart {len(S_)}, padd {len(P_)}")


# ----------------------------------------------------- fr29 register steps
def test_fr29_register_steps():
    """The chains of test_radix_steps_chain_keep_the_invariant through the
    device steps (Shoup and R'-form twiddles), starting at the top of the
    invariant, with twiddles p - 1, 1 and 0 among the random ones: the
    butterflies' residues and the step invariant (normalized, < 8p); the
    last-stage steps stay inside the store's reduce range."""
    import random as R
    from test_fr29_host import adversarial, dif_pair, mont_tw, rand_norm, shoup_tw
    F, p = FR29, FR29.P
    R.seed(3)
    normalized = lambda ls: all(x <= F.M for x in ls[:8])  # noqa: E731
    groups = [[rand_norm(8 * p) for _ in range(4)] for _ in range(300)]
    groups += [[adversarial(8 * p) for _ in range(4)] for _ in range(700)]
    groups += [[L.ones(F, 8)] * 4, [F.limbs(8 * p - 1)] * 4]
    special = [p - 1, 1, 0]
    tws = [[R.choice(special) if R.random() < 0.3 else R.randrange(p) for _ in range(4)] for _ in groups]
    for rnd in range(3):  # three chained steps (the outputs feed the next)
        gs = device(F, FR_OPS["radix4s"], [flat(*g, *[x for w in t for x in shoup_tw(w)]) for g, t in zip(groups, tws)])
        gm = device(F, FR_OPS["radix4m"], [flat(*g, *[mont_tw(w) for w in t]) for g, t in zip(groups, tws)])
        for k, (g, t) in enumerate(zip(groups, tws)):
            xv = [F.value(x) % p for x in g]
            s0, y2 = dif_pair(xv[0], xv[2], t[0])
            s1, y3 = dif_pair(xv[1], xv[3], t[1])
            want = [*dif_pair(s0, s1, t[2]), *dif_pair(y2, y3, t[3])]
            for res in (gs[k], gm[k]):
                xs = chunks(res, 9)
                assert [F.value(x) % p for x in xs] == want, (rnd, k)
                assert all(normalized(x) and F.value(x) < 8 * p for x in xs), (rnd, k)
        groups = [chunks(r, 9) for r in gs]
    last = device(F, FR_OPS["radix4last"], [flat(*g, *shoup_tw(t[1])) for g, t in zip(groups, tws)])
    r2 = device(F, FR_OPS["radix2"], [flat(g[0], g[1], *shoup_tw(t[0])) for g, t in zip(groups, tws)])
    r2l = device(F, FR_OPS["radix2last"], [flat(g[0], g[1]) for g in groups])
    for k, (g, t) in enumerate(zip(groups, tws)):
        xv = [F.value(x) % p for x in g]
        s0, y2 = dif_pair(xv[0], xv[2], 1)
        s1, y3 = dif_pair(xv[1], xv[3], t[1])
        xs = chunks(last[k], 9)
        assert [F.value(x) % p for x in xs] == [*dif_pair(s0, s1, 1), *dif_pair(y2, y3, 1)]
        assert all(F.value(x) < (1 << 261) for x in xs)
        a = chunks(r2[k], 9)
        assert [F.value(x) % p for x in a] == list(dif_pair(xv[0], xv[1], t[0]))
        assert all(normalized(x) and F.value(x) < 8 * p for x in a)
        b = chunks(r2l[k], 9)
        assert [F.value(x) % p for x in b] == list(dif_pair(xv[0], xv[1], 1))
        assert all(F.value(x) < (1 << 261) for x in b)
    print(f"fr29: {len(groups)} groups through 3 chained radix4 steps (both twiddle forms) and the last-stage steps")
