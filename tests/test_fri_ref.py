"""CPU-side checks of the FRI opening work (no GPU): tests/fri_ref.py's
BabyBear4 against the field axioms and tests/golden/fri_baby_bear.json, the
reference's FoldMatrix known answer (fri_config_unittest.cc), the prover side
against direct evaluation and against the verifier's own formulas, the
challenger, the new headers, and the argument and phase rules of
csrc/capi/fri_validate.h as a stand-alone host program under the address and
undefined-behaviour sanitizers."""
import json
import os
import subprocess

import numpy as np

import babybear_ref as B
import fri_ref as F
import poseidon2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "tachyon_amd", "csrc")
P = F.P

with open(os.path.join(ROOT, "tests", "golden", "fri_baby_bear.json")) as _f:
    GOLDEN = json.load(_f)


def rand_ext(seed, n):
    return np.random.default_rng(seed).integers(0, P, size=(n, 4), dtype=np.uint64)


def lde(seed, log_degree, cols, log_blowup):
    trace = np.random.default_rng(seed).integers(0, P, size=(1 << log_degree, cols), dtype=np.uint64)
    return B.coset_lde(trace, log_blowup, B.GENERATOR)


def honest_rounds(log_blowup):
    """{{4,2},{4,2}} with 5 columns; one point shared by all, one more on a matrix"""
    z, z2 = F.ext(5, 6, 7, 8), F.ext(9, 1, 2, 3)
    return [([lde(1, 4, 5, log_blowup), lde(2, 2, 5, log_blowup)], [[z], [z]]),
            ([lde(3, 4, 5, log_blowup), lde(4, 2, 5, log_blowup)], [[z], [z, z2]])]


def fixed_betas():
    k = 0
    while True:
        yield F.ext(k + 2, 3, 4, 5)
        k += 1


# ---- BabyBear4

def test_field_axioms_on_samples_and_at_the_bounds():
    a, b, c = rand_ext(1, 64), rand_ext(2, 64), rand_ext(3, 64)
    for x in (a, b, c):
        x[0] = P - 1                       # all-(p-1) operands
    a[1], b[1] = [0, 0, 0, P - 1], [0, P - 1, 0, 0]
    assert (F.e_mul(a, b) == F.e_mul(b, a)).all()
    assert (F.e_mul(F.e_mul(a, b), c) == F.e_mul(a, F.e_mul(b, c))).all()
    assert (F.e_mul(a, F.e_add(b, c)) == F.e_add(F.e_mul(a, b), F.e_mul(a, c))).all()
    assert (F.e_add(F.e_sub(a, b), b) == a).all() and (F.e_add(a, F.e_neg(a)) == 0).all()
    assert (F.e_mul(a, F.ONE) == a).all() and (F.e_mul(a, F.ZERO) == 0).all()
    assert (F.e_mul(a, F.e_inv(a)) == F.ONE).all()
    assert (F.e_inv(a[:4]) == F.e_pow(a[:4], F.ORDER4 - 2)).all()          # the norm formula against Fermat
    assert (F.e_inv(F.ZERO) == 0).all()                                    # the documented convention
    assert (F.e_pow(F.ext(0, 1), 4) == F.ext(F.W)).all()                   # x^4 = 11
    assert (F.e_pow(a[:4], F.ORDER4 - 1) == F.ONE).all()
    assert (F.e_mul_base(a, b[:, 0]) == F.e_mul(a, F.from_base(b[:, 0]))).all()
    assert (F.e_powers(a[2], 9)[8] == F.e_pow(a[2], 8)).all()
    # 11 is no square in BabyBear and x^2 - 11 stays irreducible over F[y]/(y^2 - 11): the ring is a field
    assert pow(F.W, (P - 1) // 2, P) == P - 1
    assert (F.from_bytes(F.to_bytes(a)) == a).all()


def test_golden_products_and_inverses():
    rec = GOLDEN["recorded"]
    a, b = np.array(rec["a"], dtype=np.uint64), np.array(rec["b"], dtype=np.uint64)
    assert F.e_mul(a, b).tolist() == rec["product"]
    assert F.e_inv(a).tolist() == rec["inverse_a"]


def test_fold_matrix_known_answer():
    """fri_config_unittest.cc: beta 28 on rows (7,1),(2,3),(5,3),(2,5)"""
    k = GOLDEN["fold_matrix"]
    v = F.from_base(np.array(k["rows"], dtype=np.uint64).reshape(-1))
    out = F.fold_matrix(F.ext(k["beta"]), v)
    assert out[:, 0].tolist() == k["expect"] == [88, 1045105093, 111548335, 1448238559]
    assert (out[:, 1:] == 0).all()


# ---- prover side

def test_opened_values_equal_direct_evaluation():
    rng = np.random.default_rng(7)
    for log_m, cols in [(0, 3), (1, 2), (3, 5), (6, 4)]:
        m = 1 << log_m
        coeffs = rng.integers(0, P, size=(m, cols), dtype=np.uint64)
        block = B.fft(coeffs, coset=B.GENERATOR)                 # evaluations at 31 w_m^r
        z = F.ext(*rng.integers(0, P, size=4))
        ys = F.interpolate_coset(block, z)
        zp = F.e_powers(z, m)                                    # direct: sum_j coeff_j z^j
        for c in range(cols):
            assert (ys[c] == F.e_sum(F.e_mul_base(zp, coeffs[:, c]))).all()


def test_prover_reduced_openings_equal_the_verifiers_at_every_index():
    for log_blowup in (1, 2):
        rounds = honest_rounds(log_blowup)
        alpha = F.ext(3, 1, 4, 1)
        opened, ro = F.reduce_openings(alpha, rounds, log_blowup)
        log_max = max(ro)
        assert sorted(ro) == [2 + log_blowup, 4 + log_blowup]
        for index in range(1 << log_max):
            info = []
            for (mats, pts), ys in zip(rounds, opened):
                per_round = []
                for mat, zs, y in zip(mats, pts, ys):
                    log_n = mat.shape[0].bit_length() - 1
                    rev = index >> (log_max - log_n)
                    row = mat[int(format(rev, "b").zfill(log_n)[::-1], 2)]
                    per_round.append((log_n, zs, y, row))
                info.append(per_round)
            got = F.verifier_reduced_openings(index, log_max, alpha, info)
            for log_n, value in got.items():
                assert (value == ro[log_n][index >> (log_max - log_n)]).all(), (index, log_n)


def test_a_point_on_the_coset_is_refused():
    mat = lde(5, 3, 2, 1)
    on_coset = F.from_base(np.uint64(F.coset_points(16)[11]))
    assert F.reduce_openings(F.ONE, [([mat], [[on_coset]])], 1) is None
    assert F.reduce_openings(F.ONE, [([mat], [[F.ext(int(F.coset_points(16)[11]), 1)]])], 1) is not None


def test_fold_matrix_equals_fold_row_at_every_index():
    for log_rows in (0, 1, 4):
        v = rand_ext(20 + log_rows, 2 << log_rows)
        beta = F.ext(11, 22, 33, 44)
        out = F.fold_matrix(beta, v)
        for r in range(1 << log_rows):
            assert (out[r] == F.fold_row(r, log_rows, beta, v[2 * r], v[2 * r + 1])).all()


def test_final_values_are_equal_for_honest_inputs_only():
    for log_blowup in (1, 2):
        rounds = honest_rounds(log_blowup)
        _, ro = F.reduce_openings(F.ext(3, 1, 4, 1), rounds, log_blowup)
        inputs = [ro[k] for k in sorted(ro, reverse=True)]
        bs = fixed_betas()
        roots, trees, vectors, final = F.commit_phase(inputs, log_blowup, lambda root: next(bs))
        assert len(roots) == 4 and final.shape == (1 << log_blowup, 4)
        assert (final == final[0]).all()
        # the queries' sibling values and the verifier's fold walk reach the same value
        for index in (0, 5, (16 << log_blowup) - 1):
            answers = F.answer_query(index, trees, vectors)
            reduced = {k: ro[k][index >> (max(ro) - k)] for k in ro}
            bs = fixed_betas()
            folded = F.verify_query(index, max(ro), [next(bs) for _ in roots], roots, answers, reduced)
            assert folded is not None and (folded == final[0]).all()
        rounds[0][0][0][3, 2] = (rounds[0][0][0][3, 2] + np.uint64(1)) % np.uint64(P)       # one corrupted row
        _, ro = F.reduce_openings(F.ext(3, 1, 4, 1), rounds, log_blowup)
        bs = fixed_betas()
        final = F.commit_phase([ro[k] for k in sorted(ro, reverse=True)], log_blowup, lambda root: next(bs))[3]
        assert not (final == final[0]).all()


def test_challenger_duplexing_and_grind():
    ch = F.DuplexChallenger("plonky3")
    ch.observe(np.arange(1, 6))
    first = ch.sample()
    want = np.zeros(16, dtype=np.uint64)
    want[:5] = np.arange(1, 6)
    state = R.permute(want[None, :], "plonky3")[0]
    assert first == int(state[15]) and ch.sample() == int(state[14])       # samples pop from the back
    ch.observe([7] * 8)                                                    # a full rate duplexes at once
    state[:8] = 7
    assert ch.state.tolist() == R.permute(state[None, :], "plonky3")[0].tolist() and not ch.inp
    verifier = ch.clone()
    witness = ch.grind(8)
    assert verifier.check_witness(8, witness)
    assert verifier.sample_ext().tolist() == ch.sample_ext().tolist()
    assert 0 <= ch.sample_bits(5) < 32


# ---- headers

USE_FRI = r"""
#include "tachyon_mi355x_fri.h"
struct BabyBear { unsigned value; };
using namespace tachyon_mi355x;
using Fri = FriOpening<BabyBear>;
bool f(const BabyBear* lde, Fri::ExtF alpha, Fri::ExtF zeta, std::vector<Fri::Digest>* commits,
       std::vector<Fri::CommitPhaseProofStep>* steps) {
  Fri fri(1, Poseidon2ExternalMatrix::kPlonky3);
  Fri::OpenedValuesForRound opened;
  if (!fri || !fri.Begin(alpha) || !fri.ReduceOpenings({{lde, 2048, 100}}, {{zeta}}, &opened)) return false;
  if (!fri.CommitPhase([&](const Fri::Digest&) { return alpha; }, commits)) return false;
  Fri::ExtF out[2];
  return fri.AnswerQuery(5, steps) && fri.final_eval()[0].value == fri.final_poly()[0][0].value &&
         BabyBear4Ops<BabyBear>(BabyBear4Op::kMul, &alpha, &zeta, out, 1) && fri.num_commits() == commits->size() &&
         fri.input(0).size() == (size_t{1} << fri.input_log_size(0)) && fri.input_device(0) && fri.num_inputs() == 1;
}
"""

USE_FIELD = r"""
#include "field/bb31x4.h"
#include "capi/fri_validate.h"
using namespace tachyon_amd;
bb31x4::Fp4 f(const bb31x4::Fp4& a, const bb31x4::Fp4& b) {
  return bb31x4::add(bb31x4::mul(a, bb31x4::inverse(b)), bb31x4::pow(bb31x4::square(bb31x4::neg(bb31x4::sub(a, b))), 5));
}
"""


def test_new_headers_compile(tmp_path):
    for name, text, inc in (("use_fri.cc", USE_FRI, INCLUDE), ("use_field.cc", USE_FIELD, CSRC)):
        src = tmp_path / name
        src.write_text(text)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# The host side of field/bb31x4.h against the golden products and inverses, and
# the argument and phase rules, in one stand-alone program.
VALIDATE_MAIN = r"""
#include <cstdio>
#include <vector>

#include "capi/fri_validate.h"
#include "field/bb31x4.h"

using namespace tachyon_amd;
using namespace tachyon_amd::fri;

static int fails = 0;
#define EXPECT(x) do { if (!(x)) { printf("FAILED: %%s\n", #x); ++fails; } } while (0)

static bb31x4::Fp4 mont(const unsigned* c) {
  return bb31x4::Fp4{{bb31::to_mont(c[0]), bb31::to_mont(c[1]), bb31::to_mont(c[2]), bb31::to_mont(c[3])}};
}

static const unsigned kA[][4] = {%(a)s};
static const unsigned kB[][4] = {%(b)s};
static const unsigned kProduct[][4] = {%(product)s};
static const unsigned kInverse[][4] = {%(inverse)s};

// exactly-sized heap arrays: a read past the end is an ASan report
static bool round_of(std::vector<const void*> ldes, std::vector<size_t> rows, std::vector<size_t> cols,
                     std::vector<const void*> points, std::vector<size_t> num, std::vector<void*> out,
                     unsigned log_blowup) {
  return round_ok(ldes.data(), rows.data(), cols.data(), rows.size(), points.data(), num.data(), out.data(),
                  log_blowup);
}

int main() {
  for (size_t i = 0; i < sizeof kA / sizeof kA[0]; ++i) {
    const bb31x4::Fp4 a = mont(kA[i]), b = mont(kB[i]);
    EXPECT(bb31x4::equal(bb31x4::mul(a, b), mont(kProduct[i])));
    EXPECT(bb31x4::equal(bb31x4::mul(b, a), mont(kProduct[i])));
    EXPECT(bb31x4::equal(bb31x4::inverse(a), mont(kInverse[i])));
    EXPECT(bb31x4::equal(bb31x4::mul(a, bb31x4::inverse(a)), bb31x4::one()));
    EXPECT(bb31x4::equal(bb31x4::square(a), bb31x4::mul(a, a)));
    EXPECT(bb31x4::equal(bb31x4::pow(a, 5), bb31x4::mul(bb31x4::square(bb31x4::square(a)), a)));
    EXPECT(bb31x4::equal(bb31x4::mul_base(a, b.c[0]), bb31x4::mul(a, bb31x4::from_base(b.c[0]))));
    EXPECT(bb31x4::equal(bb31x4::add(bb31x4::sub(a, b), b), a) && bb31x4::is_zero(bb31x4::add(a, bb31x4::neg(a))));
  }
  EXPECT(bb31x4::is_zero(bb31x4::inverse(bb31x4::zero())));
  for (unsigned v : {0u, 1u, 2u, bb31::kP - 1, bb31::kP / 11, bb31::kP / 11 + 1, 183024175u})
    EXPECT(bb31x4::mul_w(v) == (unsigned)((unsigned long long)v * 11 %% bb31::kP));

  EXPECT(!log_blowup_ok(0) && log_blowup_ok(1) && log_blowup_ok(26) && !log_blowup_ok(27));
  EXPECT(log2_exact(1) == 0 && log2_exact(2) == 1 && log2_exact(size_t(1) << 27) == 27);
  EXPECT(bit_reverse(1, 3) == 4 && bit_reverse(6, 3) == 3 && bit_reverse(0, 0) == 0);
  EXPECT(matrix_ok(2, 1, 1) && matrix_ok(size_t(1) << 27, 5, 1) && matrix_ok(4, kMaxCols, 2));
  EXPECT(!matrix_ok(8, 0, 1));                       // no columns
  EXPECT(!matrix_ok(24, 5, 1) && !matrix_ok(0, 5, 1));            // no power of two
  EXPECT(!matrix_ok(2, 5, 2) && !matrix_ok(1, 5, 1));             // below 2^log_blowup
  EXPECT(!matrix_ok(size_t(1) << 28, 5, 1) && !matrix_ok(8, kMaxCols + 1, 1));
  EXPECT(!matrix_ok(8, 5, 0) && !matrix_ok(size_t(1) << 27, 5, 27));

  int x = 0;
  const void* p = &x;
  void* o = &x;
  EXPECT(round_of({p}, {8}, {5}, {p}, {1}, {o}, 1));
  EXPECT(round_of({p, p}, {8, 32}, {5, 1}, {nullptr, p}, {0, 3}, {nullptr, o}, 2));   // no points: no buffers needed
  EXPECT(!round_of({nullptr}, {8}, {5}, {p}, {1}, {o}, 1));
  EXPECT(!round_of({p}, {8}, {5}, {nullptr}, {1}, {o}, 1) && !round_of({p}, {8}, {5}, {p}, {1}, {nullptr}, 1));
  EXPECT(!round_of({p}, {8}, {0}, {p}, {1}, {o}, 1) && !round_of({p}, {12}, {5}, {p}, {1}, {o}, 1));
  EXPECT(!round_of({p, p}, {8, 2}, {5, 5}, {p, p}, {1, 1}, {o, o}, 2));
  size_t one = 1;
  EXPECT(!round_ok(&p, &one, &one, 0, &p, &one, &o, 1));
  EXPECT(!round_ok(nullptr, &one, &one, 1, &p, &one, &o, 1) && !round_ok(&p, nullptr, &one, 1, &p, &one, &o, 1));
  EXPECT(!round_ok(&p, &one, nullptr, 1, &p, &one, &o, 1) && !round_ok(&p, &one, &one, 1, nullptr, &one, &o, 1));
  EXPECT(!round_ok(&p, &one, &one, 1, &p, nullptr, &o, 1) && !round_ok(&p, &one, &one, 1, &p, &one, nullptr, 1));

  // the phase rules: begin, inputs, commit / fold alternating, the end, the queries
  Phase ph;
  ph.log_blowup = 1;
  EXPECT(!can_add_round(ph) && !can_commit(ph) && !can_fold(ph) && !ended(ph) && !can_answer(ph, 0));
  ph.begun = true;
  EXPECT(can_add_round(ph) && !can_commit(ph));      // no input yet
  ph.has_input = true;
  ph.log_max = 3;
  EXPECT(can_commit(ph) && commit_has_work(ph) && !can_fold(ph) && !can_answer(ph, 0));
  ph.started = true;
  ph.log_size = 3;
  ph.pending = true;
  EXPECT(!can_add_round(ph) && !can_commit(ph) && can_fold(ph) && !ended(ph));
  ph.pending = false;
  ph.log_size = 2;
  EXPECT(can_commit(ph) && commit_has_work(ph) && !can_fold(ph) && !ended(ph) && !can_answer(ph, 0));
  ph.log_size = 1;
  EXPECT(can_commit(ph) && !commit_has_work(ph) && ended(ph) && can_answer(ph, 7) && !can_answer(ph, 8));
  ph.poisoned = true;
  EXPECT(!can_add_round(ph) && !can_commit(ph) && !can_fold(ph) && !ended(ph) && !can_answer(ph, 0));
  Phase small;
  small.begun = small.has_input = true;
  small.log_blowup = small.log_max = 2;
  EXPECT(can_commit(small) && !commit_has_work(small));           // nothing to fold: the phase ends at once

  EXPECT(query_pair(13, 0) == 6 && query_pair(13, 2) == 1 && query_sibling_element(13, 0) == 12 &&
         query_sibling_element(13, 1) == 7);
  EXPECT(query_num_siblings(5, 0) == 4 && query_num_siblings(5, 3) == 1 && query_total_siblings(5, 4) == 10 &&
         query_total_siblings(5, 0) == 0);
  printf("%%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def _rows(values):
    return ", ".join("{" + ", ".join(str(int(v)) for v in row) + "}" for row in values)


def test_fri_argument_checks_and_host_field_standalone_sanitized(tmp_path):
    rec = GOLDEN["recorded"]
    src = tmp_path / "fri_validate_main.cc"
    exe = tmp_path / "fri_validate_main"
    src.write_text(VALIDATE_MAIN % {"a": _rows(rec["a"]), "b": _rows(rec["b"]), "product": _rows(rec["product"]),
                                    "inverse": _rows(rec["inverse_a"])})
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-static-libasan", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


def test_header_declares_and_lib_binds_the_new_symbols():
    import re
    from tachyon_amd._lib import SIGNATURES
    text = open(os.path.join(INCLUDE, "tachyon_mi355x.h")).read()
    declared = set(re.findall(r"TACHYON_C_EXPORT[^;(]*?\b(tachyon_\w+)\s*\(", text, re.S))
    names = {n for n, _, _ in SIGNATURES}
    prefix = "tachyon_mi355x_baby_bear_fri_opening_"
    want = {prefix + s for s in ("create", "destroy", "begin", "add_round", "num_inputs", "input_log_size", "input",
                                 "input_device_ptr", "commit", "fold", "num_commits", "final_poly", "answer_query",
                                 "last_launches", "stream")} | {"tachyon_mi355x_baby_bear4_ops"}
    assert want <= declared and want <= names
