"""The lane-pair BLS12-381 G2 formulas over the 14 x 28-bit Fq
(tachyon_amd/csrc/msm/pair28.h) on the exact limb model of the device products
(tools/gen_f28.py: every column asserted below 2^64): both lanes of every
operation evaluated as the kernel does (lane 0: a0 b0 + a1 (K - b1), lane 1:
a0 b1 + a1 b0; squares as (a0 + a1)(a0 + K - a1) and a0 (2 a1)), with the
accumulator at the top of its invariant (X < 10p, Y < 6p, ZZ, ZZZ < 3p, largest
low limbs) and bases x~ << 8 up to 256p -- outputs equal madd-2008-s /
dbl-2008-s-1 over Fq2 mod p and stay inside the invariant.  The model lives
in tests/limb_model.py (PairModel); the device code itself runs on these cases
in tests/test_gpu_limb_fields.py."""
import random

from limb_model import F28, PAIR28 as M, pair_base

P, N, M28 = F28.P, F28.N, F28.M
INV = F28.INV
value = F28.value
reduce = F28.reduce
madd, dbl, point_add = M.madd, M.dbl, M.point_add
madd_ref, dbl_ref, add_ref = M.madd_ref, M.dbl_ref, M.add_ref
f2, fm = M.f2, M.fm
rand_acc, check_out = M.rand_acc, M.check_out


def base(rng, x=None):
    """a base component pair x~ << 8 with x~ (R-form, R = 2^384) canonical or lazy < 2p"""
    return pair_base(F28, rng, x, lazy=rng.random() < 0.5)


def test_pair_madd_and_dbl_at_bounds():
    rng = random.Random(11)
    for _ in range(60):
        A = rand_acc(rng)
        (x2, xv), (y2, yv) = base(rng), base(rng)
        sp, out = madd(A, x2, y2)
        assert sp == 0
        # the base as an Fq2 value: x~ 2^8 in R'' form = x 2^392 -> value x
        check_out(out, madd_ref(tuple(f2(c) for c in A), xv, yv))
        check_out(dbl(A), dbl_ref(tuple(f2(c) for c in A)))


def test_pair_madd_specials():
    rng = random.Random(12)
    for _ in range(10):
        A = rand_acc(rng)
        Af = tuple(f2(c) for c in A)
        # base = the accumulator's affine point: x2 ZZ = X, y2 ZZZ = Y -> special 2 (double)
        inv = M.finv
        xv = fm(Af[0], inv(Af[2]))
        yv = fm(Af[1], inv(Af[3]))
        (x2, _), (y2, _) = base(rng, xv), base(rng, yv)
        assert madd(A, x2, y2)[0] == 2
        (y2n, _) = base(rng, ((-yv[0]) % P, (-yv[1]) % P))
        assert madd(A, x2, y2n)[0] == 1


def test_run_start_bounds():
    rng = random.Random(13)
    for _ in range(50):
        (x2, xv), (y2, yv) = base(rng), base(rng)
        for c, want in ((x2[0], xv[0]), (x2[1], xv[1]), (y2[0], yv[0]), (y2[1], yv[1])):
            r = reduce(c)
            assert value(r) < 3 * P and value(r) * INV % P == want and all(x <= M28 for x in r[:N - 1])


def test_pair28_add_at_bounds():
    """the reductions' addition at the top of the invariant"""
    rng = random.Random(14)
    for _ in range(60):
        A, B = rand_acc(rng), rand_acc(rng)
        sp, out = point_add(A, B)
        assert sp == 0
        check_out(out, add_ref(tuple(f2(c) for c in A), tuple(f2(c) for c in B)))
