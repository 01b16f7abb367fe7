"""The Halo2 quotient without a GPU: the Python GraphEvaluator's folding rules
(the behaviour the reference's graph_evaluator_unittest.cc expects, on cases
written here), the big-integer reference (tests/quotient_ref.py) against
itself on a satisfied circuit, and the host planner's stand-alone check
(tachyon_amd/csrc/check/quotient_plan_check.cc) under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import grand_product_ref as G
import halo2_golden as H
import quotient_ref as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tachyon_amd", "csrc")
F = H.FR


def evaluator():
    from tachyon_amd.plonk_quotient import GraphEvaluator
    return GraphEvaluator("bn254_fr")


def test_constants_zero_one_two_fold_away():
    from tachyon_amd import plonk_quotient as Q
    g = evaluator()
    a = ("advice", 0, 0)
    assert g.add_expression(("const", 0)) == (Q.CONSTANT, 0, 0)
    assert g.add_expression(("const", 1)) == (Q.CONSTANT, 1, 0)
    assert g.add_expression(("const", 2)) == (Q.CONSTANT, 2, 0)
    assert g.add_expression(("const", 9)) == (Q.CONSTANT, 3, 0)
    assert g.add_expression(("const", 9)) == (Q.CONSTANT, 3, 0) and g.constants == [0, 1, 2, 9]
    assert g.calculations == []
    stored = g.add_expression(a)
    assert stored == (Q.INTERMEDIATE, 0, 0) and g.calculations == [(Q.STORE, (Q.ADVICE, 0, 0), None, ())]
    # x + 0, 0 + x, x * 1, 1 * x: the operand itself; x * 0: the zero constant
    for e in (("sum", a, ("const", 0)), ("sum", ("const", 0), a), ("product", a, ("const", 1)),
              ("product", ("const", 1), a), ("scaled", a, 1)):
        assert g.add_expression(e) == stored
    assert g.add_expression(("product", a, ("const", 0))) == (Q.CONSTANT, 0, 0)
    assert g.add_expression(("scaled", a, 0)) == (Q.CONSTANT, 0, 0)
    assert g.add_expression(("neg", ("const", 0))) == (Q.CONSTANT, 0, 0)
    assert len(g.calculations) == 1


def test_negated_constant_is_stored_as_a_constant():
    from tachyon_amd import plonk_quotient as Q
    g = evaluator()
    assert g.add_expression(("neg", ("const", 5))) == (Q.CONSTANT, 3, 0)
    assert g.constants[3] == F.p - 5 and g.calculations == []
    assert g.add_expression(("neg", ("const", 1))) == (Q.CONSTANT, 4, 0)  # -1 is no folded constant
    # a negated column is a calculation; 0 - x is a Negate, x - 0 is x, x - y a Sub
    a, b = ("advice", 0, 0), ("advice", 1, 0)
    na = g.add_expression(("neg", a))
    assert g.calculations[na[1]] == (Q.NEGATE, (Q.INTERMEDIATE, 0, 0), None, ())
    assert g.add_expression(("sum", ("const", 0), ("neg", a))) == na
    assert g.add_expression(("sum", a, ("neg", ("const", 0)))) == (Q.INTERMEDIATE, 0, 0)
    sub = g.add_expression(("sum", a, ("neg", b)))
    assert g.calculations[sub[1]][0] == Q.SUB


def test_square_double_and_operand_order():
    from tachyon_amd import plonk_quotient as Q
    g = evaluator()
    a, b = ("advice", 1, 0), ("fixed", 0, 0)
    sq = g.add_expression(("product", a, a))
    sa = (Q.INTERMEDIATE, 0, 0)
    assert g.calculations[sq[1]] == (Q.SQUARE, sa, None, ())
    for e in (("product", a, ("const", 2)), ("product", ("const", 2), a)):
        d = g.add_expression(e)
        assert g.calculations[d[1]] == (Q.DOUBLE, sa, None, ())
    # the smaller source first: intermediates by index, a constant before an intermediate
    sb = g.add_expression(b)
    assert sb[1] > sa[1]
    m1, m2 = g.add_expression(("product", b, a)), g.add_expression(("product", a, b))
    assert m1 == m2 and g.calculations[m1[1]] == (Q.MUL, sa, sb, ())
    s1 = g.add_expression(("sum", b, ("const", 7)))
    assert g.calculations[s1[1]] == (Q.ADD, (Q.CONSTANT, 3, 0), sb, ())
    # a scale is Mul(expression, constant), whatever the order rule says
    sc = g.add_expression(("scaled", a, 7))
    assert g.calculations[sc[1]] == (Q.MUL, sa, (Q.CONSTANT, 3, 0), ())


def test_repeated_query_reuses_calculation_and_rotation():
    from tachyon_amd import plonk_quotient as Q
    g = evaluator()
    q1 = g.add_expression(("instance", 2, -1))
    q2 = g.add_expression(("fixed", 2, -1))
    q3 = g.add_expression(("instance", 2, -1))
    q4 = g.add_expression(("instance", 2, 3))
    assert q1 == q3 and q1 != q2 and q4 != q1
    assert g.rotations == [-1, 3] and len(g.calculations) == 3
    assert g.calculations[q4[1]] == (Q.STORE, (Q.INSTANCE, 2, 1), None, ())
    assert g.add_expression(("challenge", 1)) == g.add_expression(("challenge", 1))
    assert g.calculations[-1] == (Q.STORE, (Q.CHALLENGE, 1, 0), None, ())


def test_construct_shapes():
    from tachyon_amd import plonk_quotient as Q
    g = Q.GraphEvaluator.for_gates(R.GATE_POLYS)
    op, init, factor, parts = g.calculations[-1]
    assert (op, init, factor) == (Q.HORNER, (Q.PREVIOUS_VALUE, 0, 0), (Q.Y, 0, 0)) and len(parts) == len(R.GATE_POLYS)
    lk = Q.GraphEvaluator.for_lookup(*R.LOOKUP_EXPRS)
    assert lk.calculations[-1][0] == Q.MUL and lk.calculations[-2][:3] == (Q.ADD, lk.calculations[-2][1], (Q.GAMMA, 0, 0))
    horners = [c for c in lk.calculations if c[0] == Q.HORNER]
    assert [(c[1], c[2]) for c in horners] == [((Q.CONSTANT, 0, 0), (Q.THETA, 0, 0))] * 2
    si, ss = Q.GraphEvaluator.for_shuffle(*R.SHUFFLE_EXPRS)
    assert si.calculations[-1][0] == Q.ADD and si.calculations[-1][2] == (Q.GAMMA, 0, 0)
    assert ss.calculations[-1][0] == Q.ADD and si is not ss
    assert Q.extended_k(16, 3) == 5 and Q.extended_k(16, 4) == 6 and Q.extended_k(16, 5) == 6 and Q.extended_k(16, 9) == 7
    z = F.from_bytes(Q.get_zeta("bn254_fr", "scroll"))
    assert z != 1 and pow(z, 3, F.p) == 1 and F.from_bytes(Q.get_zeta("bn254_fr", "pse")) == z * z % F.p
    assert z == R.get_zeta(F)
    Fb = R.field("bls12_381_fr")
    zb = Fb.from_bytes(Q.get_zeta("bls12_381_fr"))
    assert zb != 1 and pow(zb, 3, Fb.p) == 1


def golden_permutation():
    """The smallest golden circuit with a permutation: n, omega, u, sigma
    columns and a witness constant on its cycles."""
    cases = [c for c in H.circuits() if c.get("permutations_columns") and H.indicator_polys(c)]
    c = min(cases, key=lambda c: (c["n"], len(c["permutations_columns"])))
    n, omega = c["n"], int(c["omega"], 16)
    sig = [[int(h, 16) for h in col] for col in c["permutations_columns"]]
    cells = G.decode_sigmas(F, sig, omega, G.get_delta(F))
    return n, omega, H.indicator_polys(c)["u"], sig, G.cycle_constant_witness(F, cells, 77)


@pytest.mark.parametrize("cs_degree", [4, 6])
def test_reference_on_a_satisfied_circuit(cs_degree):
    """identity_at holds and the coefficients from n (cs_degree - 1) up are
    zero; on random columns (whose numerator X^n - 1 does not divide) neither does."""
    n, omega, u, sig, witness = golden_permutation()
    with O.halo2_domain():
        S = R.satisfied_system(F, n, u, omega, sig, witness, cs_degree)
        h, full, w_ext = R.h_poly(F, S)
        assert pow(w_ext, len(full) // n, F.p) == omega
        assert len(h) == n * (cs_degree - 1) and any(h)
        assert not any(full[len(h):])
        for x in R.rand(31, 2, F):
            assert R.identity_at(F, S, omega, h, x)
        B = R.random_system(F, n, cs_degree, seed=3)
        hb, fullb, _ = R.h_poly(F, B)
        assert len(fullb) > len(hb) and any(fullb[len(hb):])
        assert not R.identity_at(F, B, omega, hb, R.rand(32, 1, F)[0])


def test_quotient_plan_check_under_sanitizers(tmp_path):
    """The stand-alone program (its own main, nothing preloaded): every
    refusal, run_row(lower(g)) against the direct walk over a toy field,
    slots_needed against the live counts, the closed forms against their
    formulas."""
    exe = tmp_path / "quotient_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", str(exe),
                        os.path.join(CSRC, "check", "quotient_plan_check.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "quotient_plan_check ok" in run.stdout, run.stdout + run.stderr


def test_makefile_builds_the_check(tmp_path):
    r = subprocess.run(["make", "-s", "-n", "-C", CSRC, "../bin/quotient_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0 and "quotient_plan_check.cc" in r.stdout, r.stderr


def test_header_compiles_alone(tmp_path):
    src = tmp_path / "use.cc"
    src.write_text('#include "plonk/quotient_plan.h"\n'
                   "bool f(const tachyon_mi355x_quotient_graph& g) {\n"
                   "  return tachyon_amd::quotient_plan::graph_ok(g, tachyon_amd::quotient_plan::Sizes{});\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_program_stats_on_the_host():
    """tachyon_mi355x_quotient_program_stats needs no GPU: a chain of k sums
    multiplied together needs k slots, a stored column none, and the closed
    forms count their products."""
    from tachyon_amd import plonk_quotient as Q
    n, col = 16, b"\0" * (32 * 16)
    one = F.to_bytes(1)
    common = dict(theta=one, beta=one, gamma=one, y=one, fixed=[col, col], advice=[col, col, col], instance=[col],
                  challenges=[one])
    for k in (1, 2, 9, 10, 11, 23):
        g = Q.GraphEvaluator()
        g.add_rotation(0)
        vals = [g.add_calculation(Q.ADD, (Q.ADVICE, i % 3, 0), g.add_constant(1000 + i)) for i in range(k)]
        r = vals[0]
        for v in vals[1:]:
            r = g.add_calculation(Q.MUL, r, v)
        st = Q.quotient_program_stats("bn254_fr", n, Q.GATES, graph=g, **common)
        assert st == dict(instructions=2 * k - 1, products=k - 1, column_reads=k, slots_needed=k if k > 1 else 0)
    g = Q.GraphEvaluator()
    g.add_calculation(Q.STORE, (Q.FIXED, 1, g.add_rotation(-1)))
    assert Q.quotient_program_stats("bn254_fr", n, Q.GATES, graph=g, **common) == dict(
        instructions=1, products=0, column_reads=1, slots_needed=0)
    # the gate shape: one product per Horner part and those of the polynomials
    st = Q.quotient_program_stats("bn254_fr", n, Q.GATES, graph=Q.GraphEvaluator.for_gates(R.GATE_POLYS), **common)
    assert st["products"] == len(R.GATE_POLYS) + 5 and st["slots_needed"] <= 4
    closed = dict(common, cs_degree=4, l_first=col, l_last=col, l_active_row=col)
    st = Q.quotient_program_stats("bn254_fr", n, Q.SHUFFLE, z=[col], graph=Q.GraphEvaluator.for_shuffle(*R.SHUFFLE_EXPRS)[0],
                                  graph2=Q.GraphEvaluator.for_shuffle(*R.SHUFFLE_EXPRS)[1], **closed)
    # three folds, (1 - z) l_first, z^2, l_last (..), z(wX) S, z A, l_active (..), one Horner part each side
    assert st["products"] == 3 + 6 + 2
    c12 = b"\0" * (32 * 12)
    assert Q.quotient_program_stats("bn254_fr", 12, Q.GATES, graph=g, theta=one, beta=one, gamma=one, y=one,
                                    fixed=[c12, c12]) is None  # n is no power of two
