"""CPU-side checks of the Poseidon2 / FieldMerkleTree work (no GPU):
tests/poseidon2_ref.py pinned to the reference's known answer
(poseidon2_unittest.cc:83-104) and to tests/golden/poseidon2_baby_bear.json,
the layers as explicit matrices, the generated constants header, the openings,
the C-ABI's declarations and bindings, the C++ header, and the argument checks
of csrc/capi/merkle_tree_validate.h as a stand-alone host program under the
address and undefined-behaviour sanitizers."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import poseidon2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "tachyon_amd", "csrc")
P = R.P

with open(os.path.join(ROOT, "tests", "golden", "poseidon2_baby_bear.json")) as _f:
    GOLDEN = json.load(_f)
REF, REC = GOLDEN["reference"], GOLDEN["recorded"]


def m(r, c):
    i, j = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
    return ((1000003 * i + 7919 * j + 5) % P).astype(np.uint64)


def rand(seed, r, c):
    return np.random.default_rng(seed).integers(0, P, size=(r, c), dtype=np.uint64)


# ---- constants
def test_grain_lfsr_constants():
    ark = R.round_constants()
    assert [len(r) for r in ark] == [16] * 4 + [1] * 13 + [16] * 4
    assert ark[0][:4] == REF["ark_0_0_to_3"] and ark[4][0] == REF["ark_4_0"] and ark[20][15] == REF["ark_20_15"]
    flat = [v for r in ark for v in r]
    assert flat == REC["ark"] and len(flat) == 141 and all(0 <= v < P for v in flat)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generated_header_is_current_and_equals_the_reference_lfsr():
    gen = _load(os.path.join(ROOT, "tools", "gen_poseidon2_bb_constants.py"), "_gen_p2")
    text = open(gen.PATH).read()
    assert text == gen.render(), "run tools/gen_poseidon2_bb_constants.py"
    body = text.split("#define POSEIDON2_BB_ROUND_CONSTANTS")[1].split("inline constexpr")[0]
    consts = [int(v, 16) for v in re.findall(r"0x([0-9a-f]{8})u", body)]
    flat = [v for r in R.round_constants() for v in r]
    assert consts == [v * R.R % P for v in flat]
    assert gen.round_constants() == flat      # two restatements of the LFSR agree
    shifts = re.search(r"#define POSEIDON2_BB_INTERNAL_SHIFTS (.*)", text).group(1)
    assert tuple(int(s) for s in shifts.split(",")) == R.SHIFTS
    assert "kBeginPartial = 64;" in text and "kBeginLastFull = 77;" in text and "kNumConstants = 141;" in text


def test_params_module_agrees():
    params = _load(os.path.join(ROOT, "tachyon_amd", "params.py"), "_params_p2")
    assert params.POSEIDON2_BB_INTERNAL_SHIFTS == R.SHIFTS and params.POSEIDON2_M4 == R.M4
    assert (params.POSEIDON2_BB_WIDTH, params.POSEIDON2_BB_RATE, params.POSEIDON2_BB_DIGEST) == (16, 8, 8)
    assert (params.POSEIDON2_BB_FULL_ROUNDS, params.POSEIDON2_BB_PARTIAL_ROUNDS, params.POSEIDON2_BB_ALPHA) == (8, 13, 7)
    assert params.POSEIDON2_EXTERNAL == {"horizen": 0, "plonky3": 1}


# ---- layers as explicit matrices
def _matvec(mat, s):
    return np.array([[sum(int(mat[i, j]) * int(v[j]) for j in range(16)) % P for i in range(16)] for v in s],
                    dtype=np.uint64)


@pytest.mark.parametrize("external", ["horizen", "plonky3"])
def test_external_layer_is_its_matrix(external):
    mat = R.external_matrix(external)
    m4 = np.array(R.M4[external], dtype=np.uint64)
    for a in range(4):
        for b in range(4):
            assert (mat[4 * a:4 * a + 4, 4 * b:4 * b + 4] == (2 if a == b else 1) * m4).all()
    s = np.vstack([rand(11, 5, 16), np.full((1, 16), P - 1, dtype=np.uint64), np.eye(16, dtype=np.uint64)])
    assert (R.external_layer(s, external) == _matvec(mat, s)).all()


def test_internal_layer_is_its_matrix():
    mat = R.internal_matrix()
    rinv = pow(2, -32, P)
    for i in range(16):
        for j in range(16):
            d = 0 if i != j else (P - 2 if i == 0 else 1 << R.SHIFTS[i - 1])
            assert int(mat[i, j]) == (1 + d) * rinv % P
    s = np.vstack([rand(12, 5, 16), np.full((1, 16), P - 1, dtype=np.uint64), np.eye(16, dtype=np.uint64)])
    assert (R.internal_layer(s) == _matvec(mat, s)).all()


# ---- permutation, hash, compression
def test_known_answers():
    x = [list(range(16))]
    assert R.permute(x, "horizen")[0].tolist() == REF["horizen_permute_0_to_15"]
    p3 = R.permute(x, "plonky3")[0].tolist()
    assert p3[:4] == REF["plonky3_permute_0_to_15_lanes_0_to_3"] and p3[15] == REF["plonky3_permute_0_to_15_lane_15"]
    assert p3 == REC["plonky3_permute_0_to_15"]
    assert R.permute([[P - 1] * 16], "horizen")[0].tolist() == REC["horizen_permute_all_p_minus_1"]
    assert R.hash_rows([list(range(10))], "horizen")[0].tolist() == REF["horizen_hash_0_to_9"]
    assert R.hash_rows([list(range(17))], "plonky3")[0].tolist() == REC["plonky3_hash_0_to_16"]
    assert R.compress([list(range(8))], [list(range(8, 16))])[0].tolist() == REC["horizen_compress_0_to_7_8_to_15"]


def test_permute_is_vectorised_over_rows_and_a_bijection_on_samples():
    s = rand(13, 9, 16)
    both = R.permute(s, "horizen")
    for i in range(9):
        assert (R.permute(s[i:i + 1], "horizen")[0] == both[i]).all()
    assert len({tuple(r) for r in both.tolist()}) == 9
    assert (R.permute(s, "plonky3") != both).any()


def test_hash_overwrites_and_keeps_stale_lanes():
    row = rand(14, 1, 10)
    s = np.zeros((1, 16), dtype=np.uint64)
    s[:, :8] = row[:, :8]
    s = R.permute(s)
    s[:, :2] = row[:, 8:]                 # lanes 2..7 keep the first permutation's output
    assert (R.hash_rows(row)[0] == R.permute(s)[0, :8]).all()
    padded = np.concatenate([row, np.zeros((1, 6), dtype=np.uint64)], axis=1)
    assert (R.hash_rows(padded) != R.hash_rows(row)).any()
    assert (R.compress(row[:, :8], np.zeros((1, 8), dtype=np.uint64)) == R.permute(
        np.concatenate([row[:, :8], np.zeros((1, 8), dtype=np.uint64)], axis=1))[:, :8]).all()


def test_mont_round_trip():
    x = rand(15, 3, 7)
    assert (R.from_mont_words(R.mont_words(x)) == x).all()
    assert int(R.mont_words([1])[0]) == R.R % P
    assert R.from_bytes(R.to_bytes(x), 7).tolist() == x.tolist()


# ---- tree
def test_tree_cross_checks():
    assert R.build([np.array([[2], [1], [2], [2], [0], [0], [1], [0]])], "plonky3")[-1][0].tolist() == \
        REF["plonky3_root_8x1_21220010"]
    layers = R.build([m(8, 3), m(3, 9), m(8, 2), m(2, 17)])
    assert layers[-1][0].tolist() == REF["horizen_root_8x3_3x9_8x2_2x17"]
    assert [l.tolist() for l in layers] == REC["horizen_layers_8x3_3x9_8x2_2x17"]
    assert int(R.build([m(5, 10)])[-1][0][0]) == REF["horizen_root_5x10_word_0"]
    assert int(R.build([m(8, 3)], bit_reversed=True)[-1][0][0]) == REF["horizen_root_8x3_bit_reversed_word_0"]
    assert [l.tolist() for l in R.build([m(5, 10), m(2, 3)], "plonky3")] == REC["plonky3_layers_5x10_2x3"]
    assert [l.tolist() for l in R.build([m(4, 9)], bit_reversed=True)] == REC["horizen_layers_4x9_bit_reversed"]


def test_tree_shape_rules_from_the_definition():
    a, b, c, d = rand(21, 8, 3), rand(22, 3, 9), rand(23, 8, 2), rand(24, 2, 17)
    layers = R.build([a, b, c, d])
    assert [len(l) for l in layers] == [8, 4, 2, 1]
    zero = np.zeros((1, 8), dtype=np.uint64)
    h0 = R.hash_rows(np.concatenate([a, c], axis=1))
    assert (layers[0] == h0).all()
    l1 = R.compress(h0[0::2], h0[1::2])
    inj = np.concatenate([R.hash_rows(b), zero])
    l1 = R.compress(l1, inj)
    assert (layers[1] == l1).all()
    l2 = R.compress(R.compress(l1[0::2], l1[1::2]), R.hash_rows(d))
    assert (layers[2] == l2).all()
    assert (layers[3] == R.compress(l2[0:1], l2[1:2])).all()
    # the stable sort: equal heights keep the caller's order
    assert (R.build([c, b, a, d])[0] == R.hash_rows(np.concatenate([c, a], axis=1))).all()
    # a non-power-of-two tallest matrix: zero digests pad layer 0
    five = R.build([rand(25, 5, 10)])
    assert [len(l) for l in five] == [8, 4, 2, 1] and not five[0][5:].any() and five[0][:5].all(axis=1).all()
    one = rand(26, 1, 5)
    assert len(R.build([one])) == 1 and (R.build([one])[0] == R.hash_rows(one)).all()
    assert R.heights_ok([64, 32, 32, 5]) and not R.heights_ok([64, 32, 30]) and not R.heights_ok([5, 7])
    with pytest.raises(AssertionError):
        R.build([rand(27, 32, 3), rand(28, 30, 7)])


def test_bit_reversed_leaves_equal_the_permuted_matrix():
    for rows in (1, 2, 8, 32):
        x = rand(30 + rows, rows, 5)
        got = R.build([x], bit_reversed=True)
        want = R.build([R.bit_reverse_rows(x)])
        assert all((g == w).all() for g, w in zip(got, want))
    assert R.bit_reverse_rows(np.arange(8)).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]


@pytest.mark.parametrize("external", ["horizen", "plonky3"])
def test_every_opening_verifies(external):
    sets = [[(8, 3), (4, 9), (8, 2), (2, 17)], [(16, 10)], [(1, 4)], [(5, 10), (3, 2)], [(2, 17), (8, 3), (1, 1)]]
    for n, dims in enumerate(sets):
        mats = [rand(40 + 10 * n + i, r, c) for i, (r, c) in enumerate(dims)]
        for rev in (False, True):
            if rev and any(r & (r - 1) for r, _ in dims):
                continue
            layers = R.build(mats, external, rev)
            log_max = len(layers) - 1
            for index in range(len(layers[0])):
                opened, sib = R.open_at(mats, layers, index, rev)
                assert len(sib) == log_max and [len(o) for o in opened] == [c for _, c in dims]
                exists = all((index >> (log_max - R.ceil_log2(r))) < r for r, _ in dims)
                assert R.verify(layers[-1][0], dims, index, opened, sib, external) == exists
                if exists:
                    bad = [o.copy() for o in opened]
                    bad[-1][0] = (bad[-1][0] + np.uint64(1)) % np.uint64(P)
                    assert not R.verify(layers[-1][0], dims, index, bad, sib, external)


# ---- the boundary: declarations, bindings, headers
NEW_SYMBOLS = ["tachyon_mi355x_poseidon2_baby_bear_permute", "tachyon_mi355x_baby_bear_mul_rate"] + [
    "tachyon_mi355x_baby_bear_merkle_tree_" + s for s in
    ("create", "destroy", "build", "root", "num_layers", "layer_size", "layer", "layers_device_ptr", "open",
     "last_launches", "stream")]


def test_header_declares_and_lib_binds_the_new_symbols():
    text = open(os.path.join(INCLUDE, "tachyon_mi355x.h")).read()
    declared = set(re.findall(r"TACHYON_C_EXPORT[^;(]*?\b(tachyon_\w+)\s*\(", text, re.S))
    lib_text = open(os.path.join(ROOT, "tachyon_amd", "_lib.py")).read()
    bound = set(re.findall(r'\("(tachyon_\w+)"', lib_text))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in bound, s
    assert "TACHYON_MI355X_MERKLE_BIT_REVERSED 1u" in text


USE_TREE = r"""
#include "tachyon_mi355x_merkle_tree.h"

namespace crypto = tachyon_mi355x;
struct BabyBear {
  unsigned value;
  bool operator==(const BabyBear& other) const { return value == other.value; }
};
using Tree = crypto::FieldMerkleTree<BabyBear>;

bool f(const std::vector<BabyBear>& a, const std::vector<BabyBear>& b, Tree::Digest* commitment,
       std::vector<std::vector<BabyBear>>* openings, std::vector<Tree::Digest>* proof) {
  Tree prover_data(crypto::Poseidon2ExternalMatrix::kPlonky3);
  if (!prover_data.Build({{a.data(), 8, a.size() / 8}, {b.data(), 4, b.size() / 4}})) return false;
  *commitment = prover_data.GetRoot();
  const std::vector<std::vector<Tree::Digest>> layers = prover_data.digest_layers();
  if (layers.back()[0] != *commitment) return false;
  Tree moved = std::move(prover_data);
  return moved.CreateOpeningProof(3, openings, proof);
}

std::unique_ptr<Tree> g(const tachyon_mi355x::IcicleNTTHolder<BabyBear, tachyon_mi355x::kBabyBear>& holder,
                        const BabyBear* trace, BabyBear* lde, BabyBear shift, BabyBear* states) {
  if (!crypto::Poseidon2Permute(crypto::Poseidon2ExternalMatrix::kHorizen, states, 4)) return nullptr;
  return crypto::Commit<BabyBear>(holder, {{trace, 1024, 100}}, 1, shift, {lde});
}
"""


def test_merkle_tree_header_compiles(tmp_path):
    src = tmp_path / "use_tree.cc"
    src.write_text(USE_TREE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


VALIDATE_MAIN = r"""
#include <cstdio>
#include <vector>

#include "capi/merkle_tree_validate.h"

using namespace tachyon_amd::merkle_tree;

static int fails = 0;
#define EXPECT(x) do { if (!(x)) { printf("FAILED: %s\n", #x); ++fails; } } while (0)

// exactly-sized heap arrays: a read past the end is an ASan report
static bool plan_of(std::vector<size_t> rows, std::vector<size_t> cols, unsigned flags, Plan* p) {
  return make_plan(rows.data(), cols.data(), rows.size(), flags, p);
}

int main() {
  EXPECT(external_ok(0) && external_ok(1) && !external_ok(2) && !external_ok(-1));
  EXPECT(bit_ceil(1) == 1 && bit_ceil(2) == 2 && bit_ceil(3) == 4 && bit_ceil(1000) == 1024 && bit_ceil(1024) == 1024);
  EXPECT(ceil_log2(1) == 0 && ceil_log2(2) == 1 && ceil_log2(3) == 2 && ceil_log2(4096) == 12 && ceil_log2(4097) == 13);
  EXPECT(bit_reverse(1, 3) == 4 && bit_reverse(6, 3) == 3 && bit_reverse(0, 0) == 0 && bit_reverse(1, 10) == 512);

  Plan p;
  size_t one = 1;
  EXPECT(!make_plan(nullptr, &one, 1, 0, &p) && !make_plan(&one, nullptr, 1, 0, &p) && !make_plan(&one, &one, 1, 0, nullptr));
  EXPECT(!make_plan(&one, &one, 0, 0, &p));
  EXPECT(!plan_of({0}, {5}, 0, &p) && !plan_of({5}, {0}, 0, &p) && !plan_of({8, 0}, {3, 3}, 0, &p));
  EXPECT(!plan_of({8}, {3}, 2, &p) && !plan_of({8}, {3}, 0x80000001u, &p));
  EXPECT(!plan_of({64, 32, 30}, {5, 3, 7}, 0, &p) && !plan_of({30, 64, 32}, {7, 5, 3}, 0, &p));
  EXPECT(!plan_of({5, 7}, {1, 1}, 0, &p));
  EXPECT(!plan_of({30}, {7}, kFlagBitReversed, &p) && !plan_of({64, 30}, {5, 7}, kFlagBitReversed, &p));
  EXPECT(!plan_of({kMaxRows + 1}, {1}, 0, &p) && !plan_of({4}, {kMaxRowWords + 1}, 0, &p));
  EXPECT(!plan_of({4, 4}, {kMaxRowWords, 1}, 0, &p));
  EXPECT(!plan_of(std::vector<size_t>(kMaxGroup + 1, 8), std::vector<size_t>(kMaxGroup + 1, 2), 0, &p));
  EXPECT(plan_of(std::vector<size_t>(kMaxGroup, 8), std::vector<size_t>(kMaxGroup, 2), 0, &p));
  EXPECT(p.levels.size() == 4 && p.levels[0].count == kMaxGroup);

  // {8x3, 3x9, 8x2, 2x17}: the stable sort, one level per power of two
  EXPECT(plan_of({8, 3, 8, 2}, {3, 9, 2, 17}, 0, &p));
  EXPECT(p.log_max == 3 && p.levels.size() == 4);
  EXPECT(p.order == (std::vector<size_t>{0, 2, 1, 3}));
  EXPECT(p.levels[0].size == 8 && p.levels[0].first == 0 && p.levels[0].count == 2 && p.levels[0].rows == 8);
  EXPECT(p.levels[1].size == 4 && p.levels[1].first == 2 && p.levels[1].count == 1 && p.levels[1].rows == 3);
  EXPECT(p.levels[2].size == 2 && p.levels[2].count == 1 && p.levels[2].rows == 2);
  EXPECT(p.levels[3].size == 1 && p.levels[3].count == 0);
  EXPECT(layer_offset(p, 0) == 0 && layer_offset(p, 1) == 8 && layer_offset(p, 3) == 14 && layer_offset(p, 9) == 15);
  // a refusal leaves the plan it was given alone
  EXPECT(!plan_of({64, 32, 30}, {5, 3, 7}, 0, &p) && p.levels.size() == 4);
  EXPECT(plan_of({1}, {5}, kFlagBitReversed, &p) && p.log_max == 0 && p.levels.size() == 1 && p.levels[0].rows == 1);
  EXPECT(plan_of({5, 1, 2}, {10, 3, 9}, 0, &p) && p.log_max == 3 && p.levels[1].count == 0 && p.levels[2].rows == 2 &&
         p.levels[3].rows == 1 && p.order == (std::vector<size_t>{0, 2, 1}));
  EXPECT(plan_of({1024, 500, 16}, {10, 4, 33}, 0, &p) && p.levels.size() == 11 && p.levels[1].rows == 500 &&
         p.levels[6].rows == 16 && p.levels[5].count == 0);

  size_t r = 99;
  EXPECT(open_row(7, 3, 8, 0, &r) && r == 7);
  EXPECT(open_row(7, 3, 3, 0, &r) == false && r == 3);     // the padded part of a 3-row matrix
  EXPECT(open_row(5, 3, 3, 0, &r) && r == 2);
  EXPECT(open_row(7, 3, 2, 0, &r) && r == 1 && open_row(7, 3, 1, 0, &r) && r == 0);
  EXPECT(open_row(1, 3, 8, kFlagBitReversed, &r) && r == 4 && open_row(6, 3, 4, kFlagBitReversed, &r) && r == 3);
  EXPECT(open_row(0, 0, 1, kFlagBitReversed, &r) && r == 0);
  printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_merkle_tree_argument_checks_standalone_sanitized(tmp_path):
    src = tmp_path / "merkle_validate_main.cc"
    exe = tmp_path / "merkle_validate_main"
    src.write_text(VALIDATE_MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-static-libasan", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
