"""The shared limb model (tests/limb_model.py) pinned to the host build of the
headers, limb for limb -- the reference of tests/test_gpu_limb_fields.py tested
without a GPU: the integer formula of the products against f29.h / f28.h redc
and fr29.h mont_cxx on operands with limbs up to 30 bits and on the call-site
operands the device test sends; the quotient of reduce_shl5 / reduce, with
the device's fused and the host's two-step rounding, inside q* - 2 .. q* on
the quotient boundaries and float32 rounding midpoints; the host's own
reduce against the two-step model."""
import random

import pytest

import limb_model as L
from limb_model import F28, F29, FR29
from test_f28_host import run as f28_run  # noqa: F401  (fixtures: the host harnesses)
from test_f29_host import harness as f29_run  # noqa: F401
from test_fr29_host import run as fr29_run  # noqa: F401

OPS = ("mul", "mul_add", "mul2_add", "mul2_add5", "sqr", "sqr_add")


def fmt(op, *xs):
    return " ".join([op] + [str(t) for x in xs for t in x])


def operands_of(op, a, b, c, d, e):
    return {"mul": (a, b), "mul_add": (a, b, e), "mul2_add": (a, b, c, d), "mul2_add5": (a, b, c, d, e),
            "sqr": (a,), "sqr_add": (a, e)}[op]


def _pin_products(F, run):
    rng = random.Random(41)
    cases = []  # 3000 per family: 500 operand sets through the six ops
    for ops5 in L.random_product_cases(F, rng, 500):
        cases += [(op, operands_of(op, *ops5)) for op in OPS]
    site = L.product_cases(F, rng, 4)
    cases += [(op, ops) for op in OPS for ops in site[op]]
    out = run([fmt(op, *ops) for op, ops in cases])
    bad = [(op, ops) for (op, ops), r in zip(cases, out) if r != L.product_expected(F, op, ops)]
    assert not bad, (len(bad), bad[0])
    # the column model agrees too (it is what the lane-pair and point models run on)
    for op, ops in cases[:600]:
        a = ops[0]
        if op in ("sqr", "sqr_add"):
            assert F.redc([(a, a)], ops[1] if op == "sqr_add" else None) == L.product_expected(F, op, ops)
    return len(cases)


def test_product_formula_matches_host_f29(f29_run):  # noqa: F811
    assert _pin_products(F29, f29_run) >= 3000


def test_product_formula_matches_host_f28(f28_run):  # noqa: F811
    assert _pin_products(F28, f28_run) >= 3000


def test_product_formula_matches_host_fr29_mont(fr29_run):  # noqa: F811
    rng = random.Random(42)
    cases = [(a, b) for a, b, _, _, _ in L.random_product_cases(FR29, rng, 1000)]
    # the butterflies' widest operand (s0 + 32p - s1, limbs < 2^31.3) times a canonical twiddle
    wide = FR29.add_ksub(FR29.times(L.ones(FR29, 8), 2), FR29.K["K32"], [0] * 9)
    cases += [(wide, FR29.limbs(w)) for w in (0, 1, FR29.P - 1, FR29.R1)]
    out = fr29_run([fmt("mont", a, b) for a, b in cases])
    for (a, b), r in zip(cases, out):
        assert r == FR29.product_case(a, b), (a, b)


def _limits(F):
    return L.REDUCE_RANGE[F.name]


@pytest.mark.parametrize("F", [F29, F28, FR29], ids=lambda F: F.name)
def test_float_quotient_both_roundings_inside_contract(F):
    rng = random.Random(43)
    vmax, every = _limits(F)
    inputs = L.reduce_inputs(F, rng, vmax, every)
    assert F.kinvphi() == L.f32(1.0 / L.f32_of_int(F.P_HI + 1)) and F.P_HI + 1 == {
        "f29": 1702635872462389, "f28": F28.P_HI + 1, "fr29": L.gen_fr29.P_HI + 1}[F.name]
    differ = 0
    for v in inputs:
        qs = F.value(v) // F.P
        for fused in (False, True):
            q = F.quotient(v, fused)
            assert max(qs - 2, 0) <= q <= qs, (v, fused, q, qs)
            L.check_reduced(F, v, F.reduce(v, fused))
        differ += F.quotient(v, False) != F.quotient(v, True)
    # (float)l_top 2^W is exact (a power-of-two scaling), so the first of the two roundings
    # changes nothing: the fused and the two-step estimate are the same number
    assert differ == 0


def test_host_reduce_is_the_two_step_model(f29_run, f28_run, fr29_run):  # noqa: F811
    rng = random.Random(44)
    for F, run in ((F29, f29_run), (F28, f28_run), (FR29, fr29_run)):
        vmax, every = _limits(F)
        inputs = L.reduce_inputs(F, rng, vmax, min(every, 2000), n_random=100, n_mid=50)
        out = run([fmt("reduce", v) for v in inputs])
        for v, r in zip(inputs, out):
            assert r == F.reduce(v, fused=False), (F.name, v)
