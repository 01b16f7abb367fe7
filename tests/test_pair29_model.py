"""The lane-pair BN254 G2 formulas over the 9 x 29-bit Fq
(tachyon_amd/csrc/msm/pair29.h) on the exact limb model of the device products
(field/f29.h's columns, every column asserted below 2^64): both lanes of every
operation evaluated as the kernel does (lane 0: a0 b0 + a1 (K - b1), lane 1:
a0 b1 + a1 b0; squares as (a0 + a1)(a0 + K - a1) and a0 (2 a1)), the
accumulator at the top of madd's input invariant (X, Y < 32p, ZZ, ZZZ < 3p,
largest low limbs -- a run's first point comes in unreduced as x~ << 5) and
bases x~ << 5 < 32p -- outputs equal madd-2008-s / dbl-2008-s-1 over Fq2 mod p
and stay inside the invariant.  R' / p = 2^7.4 is small for the pair's
two-product reductions, so P and R are brought under 3p (f29::reduce_shl5)
before the products that square them.  The model lives in tests/limb_model.py
(PairModel); the device code itself runs on these cases in
tests/test_gpu_limb_fields.py."""
import random

from limb_model import F29, PAIR29 as M, pair_base

P, N = F29.P, F29.N
RP = F29.R1  # R' mod p
limbs = F29.limbs
madd, dbl, point_add = M.madd, M.dbl, M.point_add
madd_ref, dbl_ref, add_ref = M.madd_ref, M.dbl_ref, M.add_ref
f2, fm = M.f2, M.fm
OUT_BOUNDS = M.OUT_BOUNDS  # what madd and dbl leave (inside madd's input invariant, M.IN_BOUNDS)
rand_acc, check_out = M.rand_acc, M.check_out


def base(rng, x=None):
    """a base component pair x~ << 5 with x~ (R-form, R = 2^256) canonical"""
    return pair_base(F29, rng, x)


def test_pair29_madd_and_dbl_at_bounds():
    rng = random.Random(21)
    for _ in range(60):
        A = rand_acc(rng)
        (x2, xv), (y2, yv) = base(rng), base(rng)
        sp, out = madd(A, x2, y2)
        assert sp == 0
        # the base as an Fq2 value: x~ 2^5 in R' form = x 2^261 -> value x
        check_out(out, madd_ref(tuple(f2(c) for c in A), xv, yv))
        check_out(dbl(A), dbl_ref(tuple(f2(c) for c in A)))


def test_pair29_run_start_then_madd():
    """a run's first point as from_shifted leaves it (x~ << 5, Z = 1) and the next madd"""
    rng = random.Random(22)
    one = limbs(RP % P)
    for _ in range(30):
        (x2, xv), (y2, yv) = base(rng), base(rng)
        A = (x2, y2, (one, [0] * N), (one, [0] * N))
        (bx, bxv), (by, byv) = base(rng), base(rng)
        sp, out = madd(A, bx, by)
        assert sp == 0
        check_out(out, madd_ref((xv, yv, (1, 0), (1, 0)), bxv, byv))


def test_pair29_madd_specials():
    rng = random.Random(23)
    for _ in range(10):
        A = rand_acc(rng)
        Af = tuple(f2(c) for c in A)
        inv = M.finv
        xv = fm(Af[0], inv(Af[2]))
        yv = fm(Af[1], inv(Af[3]))
        (x2, _), (y2, _) = base(rng, xv), base(rng, yv)
        assert madd(A, x2, y2)[0] == 2
        (y2n, _) = base(rng, ((-yv[0]) % P, (-yv[1]) % P))
        assert madd(A, x2, y2n)[0] == 1


def test_pair29_mutant_detected():
    """the model notices a too-small site constant (16p for X, as before the
    unreduced run start): a limb wraps or a bound breaks"""
    rng = random.Random(24)
    keep = dict(M.site)
    try:
        M.site["madd_x"] = M.site["madd_y"] = "K16"
        failed = False
        for _ in range(20):
            A = rand_acc(rng)
            (x2, xv), (y2, yv) = base(rng), base(rng)
            try:
                sp, out = madd(A, x2, y2)
                check_out(out, madd_ref(tuple(f2(c) for c in A), xv, yv))
            except AssertionError:
                failed = True
                break
        assert failed
    finally:
        M.site.update(keep)


def test_pair29_add_at_bounds():
    """the reductions' addition at the top of X < 10p, Y < 6p, ZZ, ZZZ < 3p"""
    rng = random.Random(25)
    for _ in range(60):
        A, B = rand_acc(rng, OUT_BOUNDS), rand_acc(rng, OUT_BOUNDS)
        sp, out = point_add(A, B)
        assert sp == 0
        check_out(out, add_ref(tuple(f2(c) for c in A), tuple(f2(c) for c in B)))
