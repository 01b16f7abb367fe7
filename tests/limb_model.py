"""The exact Python model of the carry-free limb fields of the hot kernels
(tachyon_amd/csrc/field/f29.h, f28.h, fr29.h) and of the point formulas on
them (msm/acc29.h, acc28.h, pair29.h, pair28.h), shared by the host tests
(test_f29_host.py, test_f28_host.py, test_fr29_host.py), the lane-pair model
tests (test_pair29_model.py, test_pair28_model.py) and the device tests
(test_gpu_limb_fields.py).  Not a test file.

Two references for a product REDC(a b [+ c d]) [+ e]:
  * `redc`: the FIPS columns as the headers compute them, every column
    asserted below 2^64;
  * `product_exact`: Python integers only.  With T = A B [+ C D], R the radix
    (2^261, 2^392) and m = -T p^-1 mod R the result is the N-form of
    (T + m p) / R + E -- the limbs, not merely the residue, as long as every
    column stays below 2^64 and the top limb below 2^32 (`product_case`
    asserts both on every case it emits).

The float quotient of reduce_shl5 / reduce (`quotient`): the device compiles
(float)l_top * 2^w + (float)l_next to ONE fused multiply-add (one rounding);
the host build rounds the product and the sum separately.  Both are modelled
(`fused=`).  The product is a scaling by a power of two, hence exact, so the
two give the same number (tests/test_limb_model.py asserts it); the contract
is q in q* - 2 .. q* (q* = floor(v / p)), and outputs of the float-quotient
operations are still compared by contract (residue, N-form, < 3p), not limb
for limb: the multiply by 1 / p_hi and its rounding belong to the compiler.
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_f28  # noqa: E402
import gen_f29_constants  # noqa: E402
import gen_fr29  # noqa: E402


def f32(x):
    """x (a double) rounded to float32"""
    return struct.unpack("f", struct.pack("f", x))[0]


def f32_of_int(x):
    """(float)x of a non-negative integer: round to nearest, ties to even"""
    if x < (1 << 24):
        return float(x)
    e = x.bit_length() - 24
    q, r, half = x >> e, x & ((1 << e) - 1), 1 << (e - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return float(q << e)


class LimbField:
    """One limb field: N limbs of W bits, radix 2^(N W)."""

    def __init__(self, name, p, n, w, words, consts, one_bound_k):
        self.name, self.P, self.N, self.W, self.WORDS = name, p, n, w, words
        self.M = (1 << w) - 1
        self.RADIX = 1 << (n * w)
        self.R1 = self.RADIX % p            # 1 in the field's Montgomery form
        self.INV = pow(self.RADIX, -1, p)
        self.PINV = (-pow(p, -1, 1 << w)) % (1 << w)
        self.PINV32 = pow(p, -1, 1 << 32)
        self.PL = self.limbs(p)
        self.SHIFT = n * w - 32 * words     # x~ << SHIFT brings an R-form value to this form
        self.TOP_SHIFT = w * (n - 2)        # the float quotient looks at v >> TOP_SHIFT
        self.P_HI = p >> self.TOP_SHIFT
        self.K = {k: self.raised(*km) for k, km in consts.items()}
        self.ZERO_K = one_bound_k           # is_zero_mod_p: x < ZERO_K p
        self.ONE = self.limbs(self.R1)

    # ---- representation ----
    def limbs(self, v):
        """N-form limbs of v (limbs 0..N-2 exact, the top limb the rest)"""
        return [(v >> (self.W * i)) & self.M for i in range(self.N - 1)] + [v >> (self.W * (self.N - 1))]

    def value(self, ls):
        return sum(x << (self.W * i) for i, x in enumerate(ls))

    def n_form(self, ls):
        return all(0 <= x <= self.M for x in ls[:self.N - 1]) and 0 <= ls[self.N - 1] < (1 << 32)

    def words(self, v):
        return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(self.WORDS)]

    def raised(self, k, m):
        """k p with every low limb raised by m 2^W (borrowed from the limb above)"""
        s = self.limbs(k * self.P)
        out = ([s[0] + m * (1 << self.W)] + [s[i] + m * (1 << self.W) - m for i in range(1, self.N - 1)]
               + [s[self.N - 1] - m])
        assert self.value(out) == k * self.P and all(0 <= x < (1 << 32) for x in out)
        return out

    def top_rep(self, v, bound):
        """The representative v + k p below bound * p with the largest low limbs
        (the widest columns), as N-form limbs."""
        best = None
        for k in range(bound):
            w = v + k * self.P
            if w >= bound * self.P:
                break
            s = sum(self.limbs(w)[:self.N - 1])
            if best is None or s > best[0]:
                best = (s, w)
        return self.limbs(best[1])

    # ---- limb-wise helpers (32-bit registers: a result must not wrap) ----
    @staticmethod
    def u32(ls):
        assert all(0 <= x < (1 << 32) for x in ls), "limb wrapped"
        return ls

    def ksub(self, K, x):
        return self.u32([k - v for k, v in zip(K, x)])

    def add(self, a, b):
        return self.u32([x + y for x, y in zip(a, b)])

    def add_ksub(self, a, K, x):
        return self.u32([u + (k - v) for u, k, v in zip(a, K, x)])

    def ksub2(self, K, a, b):
        return self.u32([k - x - 2 * y for k, x, y in zip(K, a, b)])

    def times(self, a, k):
        return self.u32([x * k for x in a])

    def normalize(self, a):
        r, c = list(a), 0
        for i in range(self.N - 1):
            t = r[i] + c
            r[i], c = t & self.M, t >> self.W
        r[self.N - 1] += c
        return r

    # ---- products ----
    def redc(self, pairs, e=None, digits=None):
        """the headers' redc: columns of the products, the FIPS digits, e added
        to the output columns; every column asserted below 2^64"""
        N, W, M, PL = self.N, self.W, self.M, self.PL
        acc, m, r = 0, [0] * N, [0] * N
        for k in range(2 * N - 1):
            for a, b in pairs:
                for i in range(N):
                    if 0 <= k - i < N:
                        acc += a[i] * b[k - i]
            for i in range(N):
                if i < k and 0 < k - i < N:
                    acc += m[i] * PL[k - i]
            if k < N:
                m[k] = ((acc & 0xFFFFFFFF) * self.PINV) & M
                acc += m[k] * PL[0]
            else:
                if e is not None:
                    acc += e[k - N]
                r[k - N] = acc & M
            assert acc < (1 << 64), "column overflow"
            acc >>= W
        r[N - 1] = acc + (e[N - 1] if e is not None else 0)
        if digits is not None:
            digits[:] = m
        return self.u32(r)

    def mul(self, a, b, e=None):
        return self.redc([(a, b)], e)

    def mul2(self, a, b, c, d, e=None):
        return self.redc([(a, b), (c, d)], e)

    def product_exact(self, a, b, c=None, d=None, e=None):
        """N-form of (T + m p) / R + E from Python integers alone"""
        T = self.value(a) * self.value(b) + (self.value(c) * self.value(d) if c is not None else 0)
        m = (-T * pow(self.P, -1, self.RADIX)) % self.RADIX
        q, rem = divmod(T + m * self.P, self.RADIX)
        assert rem == 0
        return self.limbs(q + (self.value(e) if e is not None else 0))

    def columns_fit(self, pairs):
        """A sufficient bound, cheaply: the exact column sums of the operand
        products (one big multiplication on limbs spread 80 bits apart) plus
        the most the N digit products and the carry can add stay below 2^64."""
        spread = lambda x: sum(t << (80 * i) for i, t in enumerate(x))  # noqa: E731
        cols = sum(spread(a) * spread(b) for a, b in pairs)
        widest = max((cols >> (80 * k)) & ((1 << 80) - 1) for k in range(2 * self.N - 1))
        return widest + self.N * self.M * self.M + (1 << (64 - self.W)) + (1 << 32) < (1 << 64)

    def product_case(self, a, b, c=None, d=None, e=None):
        """The expected limbs of REDC(a b [+ c d]) [+ e], with the product's
        preconditions asserted on the case: every column below 2^64 (the cheap
        sufficient bound, else the exact columns of `redc`, which asserts) and
        the result's top limb below 2^32.  Nothing is filtered: an operand set
        outside the preconditions is a bug of the caller."""
        pairs = [(a, b)] + ([(c, d)] if c is not None else [])
        for x in (a, b, c, d, e):
            assert x is None or (len(x) == self.N and all(0 <= t < (1 << 32) for t in x)), "not a limb register"
        r = self.product_exact(a, b, c, d, e)
        if not self.columns_fit(pairs):
            assert self.redc(pairs, e) == r
        assert self.n_form(r), "top limb wraps"
        return r

    def force_digits(self, a, b, target, c=None, d=None):
        """b with its limbs 0..N-1 replaced so that every Montgomery digit of
        REDC(a b [+ c d]) equals target (a[0] odd): digit k is fixed by column
        k, in which b[k] enters once, as a[0] b[k]."""
        N, W, M = self.N, self.W, self.M
        assert a[0] & 1
        b = list(b)
        a0inv = pow(a[0], -1, 1 << W)
        want = (target * pow(self.PINV, -1, 1 << W)) & M  # the column's low W bits for that digit
        acc, m = 0, [0] * N
        for k in range(N):
            s = acc
            for i in range(1, N):
                if 0 <= k - i < N:
                    s += a[i] * b[k - i]
            if c is not None:
                for i in range(N):
                    if 0 <= k - i < N:
                        s += c[i] * d[k - i]
            for i in range(N):
                if i < k and 0 < k - i < N:
                    s += m[i] * self.PL[k - i]
            b[k] = ((want - s) * a0inv) & M
            acc = s + a[0] * b[k]
            m[k] = ((acc & 0xFFFFFFFF) * self.PINV) & M
            assert m[k] == target
            acc = (acc + m[k] * self.PL[0]) >> W
        return b

    def rippling_addend(self, r):
        """an addend e whose sum with the product output r (limbs before e)
        carries out of limb 0 through every low limb into the top limb"""
        return [self.M - r[0] + 1] + [self.M - x for x in r[1:self.N - 1]] + [0]

    # ---- the float quotient ----
    def kinvphi(self):
        return f32(1.0 / f32_of_int(self.P_HI + 1))

    def quotient(self, v, fused):
        """q of reduce_shl5 / reduce on limbs v: fused = one rounding of
        (float)l_top 2^W + (float)l_next (the device), else two (the host)"""
        hi, lo = f32_of_int(v[self.N - 1]), f32_of_int(v[self.N - 2])
        if fused:
            vf = f32_of_int(int(hi) * (1 << self.W) + int(lo))
        else:
            vf = f32(f32(hi * float(1 << self.W)) + lo)
        return max(int(f32(vf * self.kinvphi())) - 1, 0)

    def reduce(self, v, fused=False):
        """value - q p with signed carries: N-form, < 3p"""
        q = self.quotient(v, fused)
        r, carry = [0] * self.N, 0
        for i in range(self.N):
            t = v[i] + carry - q * self.PL[i]
            r[i] = t & self.M if i < self.N - 1 else t
            carry = t >> self.W
        assert r[self.N - 1] >= 0
        return r

    def midpoint_tops(self, vmax, count, rng):
        """(l_top, l_next) pairs with l_top 2^W + l_next on, one below and one
        above a float32 rounding midpoint, values below vmax: where the fused
        and the two-step rounding can disagree"""
        out = []
        hi_max = vmax >> (self.W * (self.N - 1))
        while len(out) < count:
            hi = rng.randrange(1, max(2, min(hi_max, 1 << 24)))
            x = hi << self.W
            ulp = 1 << (x.bit_length() - 24)
            if ulp < 4:
                continue
            # a multiple of ulp plus half an ulp, reached with l_next < 2^W
            k = rng.randrange(max(1, (1 << self.W) // ulp))
            mid = k * ulp + ulp // 2
            for lo in (mid - 1, mid, mid + 1):
                if 0 <= lo <= self.M:
                    out.append((hi, lo))
        return out

    def is_zero(self, a):
        return self.value(a) % self.P == 0

    # ---- single-lane points: affine arithmetic and accumulators ----
    def affine_add(self, Pa, Pb):
        p = self.P
        if Pa is None:
            return Pb
        if Pb is None:
            return Pa
        (x1, y1), (x2, y2) = Pa, Pb
        if x1 == x2:
            if (y1 + y2) % p == 0:
                return None
            lam = 3 * x1 * x1 * pow(2 * y1, -1, p) % p
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (lam * lam - x1 - x2) % p
        return x3, (lam * (x1 - x3) - y1) % p

    def affine_mul(self, k, Pt):
        R = None
        while k:
            if k & 1:
                R = self.affine_add(R, Pt)
            Pt = self.affine_add(Pt, Pt)
            k >>= 1
        return R

    def acc(self, pt, z, bx=10, by=3, bz=3):
        """XYZZ accumulator of affine pt with Z = z, representatives at the top
        of the invariant X < bx p, Y < by p, ZZ, ZZZ < bz p (4 N limbs)"""
        p = self.P
        x, y = pt
        zz, zzz = z * z % p, z * z * z % p
        m = lambda v: v * self.R1 % p  # noqa: E731
        return (self.top_rep(m(x * zz % p), bx) + self.top_rep(m(y * zzz % p), by) + self.top_rep(m(zz), bz)
                + self.top_rep(m(zzz), bz))

    def point_of(self, res):
        """(special, affine point or None, component values, limbs) of a result
        [special, X limbs, Y limbs, ZZ limbs, ZZZ limbs]"""
        p, N = self.P, self.N
        sp, v = res[0], res[1:]
        X, Y, ZZ, ZZZ = (self.value(v[N * i:N * i + N]) for i in range(4))
        if ZZ % p == 0:
            return sp, None, (X, Y, ZZ, ZZZ), v
        x = X * self.INV * pow(ZZ * self.INV, -1, p) % p
        y = Y * self.INV * pow(ZZZ * self.INV, -1, p) % p
        return sp, (x, y), (X, Y, ZZ, ZZZ), v

    def base_limbs(self, x):
        """x~ << SHIFT of the canonical R-form x~ = x 2^(32 WORDS) mod p"""
        return self.limbs(((x << (32 * self.WORDS)) % self.P) << self.SHIFT)


F29 = LimbField("f29", gen_f29_constants.P, 9, 29, 8,
                {"K4": (4, 1), "K8": (8, 4), "K8R1": (8, 1), "K16": (16, 1), "K33": (33, 1), "K32R3": (32, 3)}, 64)
F28 = LimbField("f28", gen_f28.P, 14, 28, 12,
                {"K4": (4, 1), "K8": (8, 3), "K16": (16, 1), "K16R2": (16, 2), "K32": (32, 1), "K32R3": (32, 3),
                 "K257": (257, 1)}, 32)
FR29 = LimbField("fr29", gen_fr29.P, 9, 29, 8, {"K16": (16, 1), "K32": (32, 2)}, 0)
# the generators' constants are these
assert F28.K["K8"] == gen_f28.K8 and F28.K["K32R3"] == gen_f28.K32R3 and F28.PINV == gen_f28.PINV
assert FR29.K["K32"] == gen_fr29.K32 and FR29.P_HI == gen_fr29.P_HI
# the base negations of msm/msm_acc.h (repack_y): 33p - y~ << 5 and 257p - y~ << 8
NEG_BASE = {"f29": F29.K["K33"], "f28": F28.K["K257"]}
# curve generators (y^2 = x^3 + 3, y^2 = x^3 + 4)
GEN = {"f29": (1, 2),
       "f28": (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
               0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)}


def point_cases(F, rng, n_pairs):
    """The cases of test_point_formulas_at_bounds: (op, operand limb lists,
    expected affine point or None, expected special) for madd / add / dbl /
    start on accumulators at the top of the invariant, bases shifted and
    negated the way the kernels do it, and the special cases with the
    accumulator given as different representatives of the same residue."""
    p = F.P
    neg = NEG_BASE[F.name]
    lazy = F.name == "f28"  # BLS12-381 R-form words may be lazy (< 2p)
    pts = [F.affine_mul(rng.randrange(1, 1 << 64), GEN[F.name]) for _ in range(2 * n_pairs)]
    cases = []
    rform = lambda v: (v << (32 * F.WORDS)) % p  # noqa: E731
    sh = F.SHIFT
    for i in range(0, 2 * n_pairs, 2):
        A, B = pts[i], pts[i + 1]
        za, zb = rng.randrange(1, p), rng.randrange(1, p)
        acc_a, acc_b = F.acc(A, za), F.acc(B, zb)
        xt, yt = rform(B[0]), rform(B[1])
        xa, ya = rform(A[0]), rform(A[1])
        nB, nA = (B[0], p - B[1]), (A[0], p - A[1])
        cases.append(("madd", acc_a + F.limbs(xt << sh) + F.limbs(yt << sh), F.affine_add(A, B), 0))
        if lazy:
            cases.append(("madd", acc_a + F.limbs((xt + p) << sh) + F.limbs((yt + p) << sh), F.affine_add(A, B), 0))
        cases.append(("madd", acc_a + F.limbs(xt << sh) + F.limbs((p - yt) << sh), F.affine_add(A, nB), 0))
        # the kernel's limb-wise negation (K - y~ << SHIFT in raised limbs), y~ = 0 the top of its bound
        cases.append(("madd", acc_a + F.limbs(xt << sh) + F.ksub(neg, F.limbs(yt << sh)), F.affine_add(A, nB), 0))
        cases.append(("madd", acc_a + F.limbs(xa << sh) + F.ksub(neg, F.limbs(ya << sh)), None, 1))
        # specials: base = acc point (the caller doubles), base = -acc (identity)
        cases.append(("madd", acc_a + F.limbs(xa << sh) + F.limbs(ya << sh), None, 2))
        cases.append(("madd", acc_a + F.limbs(xa << sh) + F.limbs((p - ya) << sh), None, 1))
        cases.append(("add", acc_a + acc_b, F.affine_add(A, B), 0))
        cases.append(("add", acc_a + F.acc(A, zb), None, 2))
        cases.append(("add", acc_a + F.acc(nA, zb), None, 1))
        cases.append(("dbl", acc_a, F.affine_add(A, A), 0))
        st = (xt + p, yt + p) if lazy else (xt, yt)
        cases.append(("start", F.limbs(st[0] << sh) + F.limbs(st[1] << sh), B, 0))
    return cases


# ---- single-lane point formulas on the limb model (msm/acc29.h, acc28.h: no
# float quotient in madd / add / dbl, so the device result is these limbs) ----
def acc_madd(F, A, x2, y2):
    X, Y, ZZ, ZZZ = A
    K = F.K
    Pv = F.mul(x2, ZZ, F.ksub(K["K16"], X))
    R = F.mul(y2, ZZZ, F.ksub(K["K4"], Y))
    if F.is_zero(Pv):
        return (2 if F.is_zero(R) else 1), A
    PP = F.mul(Pv, Pv)
    PPP = F.mul(Pv, PP)
    Q = F.mul(X, PP)
    X3 = F.mul(R, R, F.ksub2(K["K8"], PPP, Q))
    T = F.add_ksub(Q, K["K16"], X3)
    Y3 = F.mul2(R, T, F.ksub(K["K4"], Y), PPP)
    return 0, (X3, Y3, F.mul(ZZ, PP), F.mul(ZZZ, PPP))


def acc_add(F, A, B):
    X1, Y1, ZZ1, ZZZ1 = A
    X2, Y2, ZZ2, ZZZ2 = B
    K = F.K
    U1, S1 = F.mul(X1, ZZ2), F.mul(Y1, ZZZ2)
    Pv = F.mul(X2, ZZ1, F.ksub(K["K4"], U1))
    R = F.mul(Y2, ZZZ1, F.ksub(K["K4"], S1))
    if F.is_zero(Pv):
        return (2 if F.is_zero(R) else 1), A
    PP = F.mul(Pv, Pv)
    PPP = F.mul(Pv, PP)
    Q = F.mul(U1, PP)
    X3 = F.mul(R, R, F.ksub2(K["K8"], PPP, Q))
    T = F.add_ksub(Q, K["K16"], X3)
    Y3 = F.mul2(R, T, F.ksub(K["K4"], S1), PPP)
    return 0, (X3, Y3, F.mul(F.mul(ZZ1, ZZ2), PP), F.mul(F.mul(ZZZ1, ZZZ2), PPP))


def acc_dbl(F, A):
    X, Y, ZZ, ZZZ = A
    K = F.K
    U = F.times(Y, 2)
    V = F.mul(U, U)
    Wv = F.mul(U, V)
    S = F.mul(X, V)
    Mv = F.mul(X, F.times(X, 3))
    X3 = F.mul(Mv, Mv, F.ksub2(K["K8"], [0] * F.N, S))
    Y3 = F.mul2(Mv, F.add_ksub(S, K["K16"], X3), F.ksub(K["K4"], Wv), Y)
    return X3, Y3, F.mul(V, ZZ), F.mul(Wv, ZZZ)


# ---- lane-pair values: (c0 limbs, c1 limbs) ----
class PairModel:
    """msm/pair29.h / pair28.h on the limb model: both lanes of every operation
    evaluated as the kernel does (lane 0: a0 b0 + a1 (K - b1), lane 1: a0 b1 +
    a1 b0; squares as (a0 + a1)(a0 + K - a1) and a0 (2 a1)).  `site` names the
    constants and reductions in which the two headers differ."""

    def __init__(self, F, site, in_bounds, out_bounds):
        self.F, self.site = F, dict(site)
        self.IN_BOUNDS, self.OUT_BOUNDS = in_bounds, out_bounds

    def pmul(self, a, b, K, e=None):
        F = self.F
        (a0, a1), (b0, b1) = a, b
        return (F.mul2(a0, b0, a1, F.ksub(K, b1), e[0] if e else None), F.mul2(a0, b1, a1, b0, e[1] if e else None))

    def psqr_operands(self, a, K):
        F = self.F
        a0, a1 = a
        return (F.add(a0, a1), F.add(a0, F.ksub(K, a1))), (a0, F.times(a1, 2))

    def psqr(self, a, K, e=None):
        F = self.F
        (x0, y0), (x1, y1) = self.psqr_operands(a, K)
        return (F.mul(x0, y0, e[0] if e else None), F.mul(x1, y1, e[1] if e else None))

    def pksub(self, K, x):
        return (self.F.ksub(K, x[0]), self.F.ksub(K, x[1]))

    def pksub2(self, K, a, b):
        return (self.F.ksub2(K, a[0], b[0]), self.F.ksub2(K, a[1], b[1]))

    def padd_ksub(self, a, K, x):
        return (self.F.add_ksub(a[0], K, x[0]), self.F.add_ksub(a[1], K, x[1]))

    def pred(self, a, fused=False):
        return (self.F.reduce(a[0], fused), self.F.reduce(a[1], fused))

    def pnorm_times(self, a, k):
        F = self.F
        return (F.normalize(F.times(a[0], k)), F.normalize(F.times(a[1], k)))

    def pzero(self, a):
        return self.F.is_zero(a[0]) and self.F.is_zero(a[1])

    def _k(self, name):
        return self.F.K[self.site[name]]

    def start(self, x2, y2, fused=False):
        one, nil = self.F.ONE, [0] * self.F.N
        if self.site["start_reduces"]:
            x2, y2 = self.pred(x2, fused), self.pred(y2, fused)
        return (x2, y2, (one, nil), (one, nil))

    def madd(self, A, x2, y2, fused=False):
        K = self.F.K
        X, Y, ZZ, ZZZ = A
        Pv = self.pmul(x2, ZZ, K["K4"], self.pksub(self._k("madd_x"), X))
        R = self.pmul(y2, ZZZ, K["K4"], self.pksub(self._k("madd_y"), Y))
        if self.site["madd_reduces"]:
            Pv, R = self.pred(Pv, fused), self.pred(R, fused)
        if self.pzero(Pv):
            return (2 if self.pzero(R) else 1), A
        PP = self.psqr(Pv, self._k("madd_pp"))
        PPP = self.pmul(Pv, PP, K["K4"])
        Q = self.pmul(X, PP, K["K4"])
        Wv = self.pmul(Y, PPP, K["K4"])
        X3 = self.psqr(R, self._k("x3"), self.pksub2(K["K8"], PPP, Q))
        T = self.padd_ksub(Q, K["K16"], X3)
        Y3 = self.pmul(R, T, K["K32R3"], self.pksub(K["K4"], Wv))
        return 0, (X3, Y3, self.pmul(ZZ, PP, K["K4"]), self.pmul(ZZZ, PPP, K["K4"]))

    def dbl(self, A, fused=False):
        K = self.F.K
        X, Y, ZZ, ZZZ = A
        if self.site["dbl_reduces"]:
            X, Y = self.pred(X, fused), self.pred(Y, fused)
        U = self.pnorm_times(Y, 2)
        V = self.psqr(U, self._k("dbl_v"))
        Wv = self.pmul(U, V, K["K4"])
        S = self.pmul(X, V, K["K4"])
        Mv = self.pmul(X, self.pnorm_times(X, 3), self._k("dbl_m"))
        WY = self.pmul(Wv, Y, self._k("dbl_wy"))
        zero = [0] * self.F.N
        X3 = self.psqr(Mv, K["K4"], self.pksub2(K["K8"], (zero, zero), S))
        Y3 = self.pmul(Mv, self.padd_ksub(S, K["K16"], X3), K["K32R3"], self.pksub(K["K4"], WY))
        return X3, Y3, self.pmul(V, ZZ, K["K4"]), self.pmul(Wv, ZZZ, K["K4"])

    def point_add(self, A, B, fused=False):
        K = self.F.K
        X1, Y1, ZZ1, ZZZ1 = A
        X2, Y2, ZZ2, ZZZ2 = B
        U1 = self.pmul(X1, ZZ2, K["K4"])
        S1 = self.pmul(Y1, ZZZ2, K["K4"])
        Pv = self.pmul(X2, ZZ1, K["K4"], self.pksub(K["K4"], U1))
        R = self.pmul(Y2, ZZZ1, K["K4"], self.pksub(K["K4"], S1))
        if self.site["add_reduces_r"]:
            R = self.pred(R, fused)
        if self.pzero(Pv):
            return (2 if self.pzero(R) else 1), A
        PP = self.psqr(Pv, self._k("add_pp"))
        PPP = self.pmul(Pv, PP, K["K4"])
        Q = self.pmul(U1, PP, K["K4"])
        Wv = self.pmul(S1, PPP, K["K4"])
        X3 = self.psqr(R, self._k("x3"), self.pksub2(K["K8"], PPP, Q))
        T = self.padd_ksub(Q, K["K16"], X3)
        Y3 = self.pmul(R, T, K["K32R3"], self.pksub(K["K4"], Wv))
        return 0, (X3, Y3, self.pmul(self.pmul(ZZ1, ZZ2, K["K4"]), PP, K["K4"]),
                   self.pmul(self.pmul(ZZZ1, ZZZ2, K["K4"]), PPP, K["K4"]))

    # exact Fq2 algebra (u^2 = -1), values mod p of the Montgomery-form components
    def f2(self, v):
        F = self.F
        return (F.value(v[0]) * F.INV % F.P, F.value(v[1]) * F.INV % F.P)

    def fm(self, a, b):
        p = self.F.P
        return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def fs(self, a, b):
        p = self.F.P
        return ((a[0] - b[0]) % p, (a[1] - b[1]) % p)

    def fa(self, a, b):
        p = self.F.P
        return ((a[0] + b[0]) % p, (a[1] + b[1]) % p)

    def finv(self, a):
        p = self.F.P
        return self.fm((a[0], (-a[1]) % p), (pow((a[0] ** 2 + a[1] ** 2) % p, -1, p), 0))

    def madd_ref(self, A, x2, y2):
        fm, fs, fa = self.fm, self.fs, self.fa
        X, Y, ZZ, ZZZ = A
        Pv = fs(fm(x2, ZZ), X)
        R = fs(fm(y2, ZZZ), Y)
        PP = fm(Pv, Pv)
        PPP = fm(Pv, PP)
        Q = fm(X, PP)
        X3 = fs(fs(fm(R, R), PPP), fa(Q, Q))
        Y3 = fs(fm(R, fs(Q, X3)), fm(Y, PPP))
        return X3, Y3, fm(ZZ, PP), fm(ZZZ, PPP)

    def dbl_ref(self, A):
        fm, fs, fa = self.fm, self.fs, self.fa
        X, Y, ZZ, ZZZ = A
        U = fa(Y, Y)
        V = fm(U, U)
        Wv = fm(U, V)
        S = fm(X, V)
        XX = fm(X, X)
        Mv = fa(fa(XX, XX), XX)
        X3 = fs(fm(Mv, Mv), fa(S, S))
        Y3 = fs(fm(Mv, fs(S, X3)), fm(Wv, Y))
        return X3, Y3, fm(V, ZZ), fm(Wv, ZZZ)

    def add_ref(self, A, B):
        fm, fs, fa = self.fm, self.fs, self.fa
        X1, Y1, ZZ1, ZZZ1 = A
        X2, Y2, ZZ2, ZZZ2 = B
        U1, S1 = fm(X1, ZZ2), fm(Y1, ZZZ2)
        Pv = fs(fm(X2, ZZ1), U1)
        R = fs(fm(Y2, ZZZ1), S1)
        PP = fm(Pv, Pv)
        PPP = fm(Pv, PP)
        Q = fm(U1, PP)
        X3 = fs(fs(fm(R, R), PPP), fa(Q, Q))
        Y3 = fs(fm(R, fs(Q, X3)), fm(S1, PPP))
        return X3, Y3, fm(fm(ZZ1, ZZ2), PP), fm(fm(ZZZ1, ZZZ2), PPP)

    def rand_acc(self, rng, bounds=None):
        F = self.F
        bounds = bounds or self.IN_BOUNDS
        comps = [(rng.randrange(F.P), rng.randrange(F.P)) for _ in range(4)]
        return tuple((F.top_rep(c[0] * F.R1 % F.P, b), F.top_rep(c[1] * F.R1 % F.P, b)) for c, b in zip(comps, bounds))

    def check_out(self, A, want, bounds=None):
        F = self.F
        got = tuple(self.f2(c) for c in A)
        assert got == want
        for (c0, c1), b in zip(A, bounds or self.OUT_BOUNDS):
            for c in (c0, c1):
                assert all(x <= F.M for x in c[:F.N - 1]) and F.value(c) < b * F.P


PAIR29 = PairModel(F29, {"start_reduces": False, "madd_x": "K33", "madd_y": "K33", "madd_reduces": True,
                         "madd_pp": "K4", "x3": "K4", "dbl_reduces": True, "dbl_v": "K4", "dbl_m": "K16",
                         "dbl_wy": "K4", "add_reduces_r": True, "add_pp": "K8R1"},
                   in_bounds=(32, 32, 3, 3), out_bounds=(10, 6, 3, 3))
PAIR28 = PairModel(F28, {"start_reduces": True, "madd_x": "K16", "madd_y": "K8", "madd_reduces": False,
                         "madd_pp": "K32", "x3": "K16", "dbl_reduces": False, "dbl_v": "K16", "dbl_m": "K32",
                         "dbl_wy": "K8", "add_reduces_r": False, "add_pp": "K16"},
                   in_bounds=(10, 6, 3, 3), out_bounds=(10, 6, 3, 3))


def pair_base(F, rng, x=None, lazy=False):
    """a base component pair x~ << SHIFT with x~ (R-form) canonical, or lazy (< 2p) with `lazy`"""
    x = x if x is not None else (rng.randrange(F.P), rng.randrange(F.P))
    add_p = F.P if lazy else 0
    return tuple(F.limbs((((c << (32 * F.WORDS)) % F.P) + add_p) << F.SHIFT) for c in x), x


# ---- product operands at the bounds of their call sites ----
def ones(F, bound):
    """the largest value below bound p whose low limbs are all ones"""
    top = ((bound * F.P) >> (F.W * (F.N - 1))) - 1
    assert top >= 0
    return [F.M] * (F.N - 1) + [top]


def product_cases(F, rng, n_random):
    """{op: [operand tuples]} for mul (a, b), mul_add (a, b, e), mul2_add
    (a, b, c, d), mul2_add5 (a, b, c, d, e), sqr (a), sqr_add (a, e): the
    operands of every product in msm/acc29.h / acc28.h (madd, add, dbl) and of
    the lane-pair products of msm/pair29.h / pair28.h, built with the limb-wise
    helpers from values at the top of their documented bounds (all-ones low
    limbs), from random values over the same ranges and from zero; operands
    that force every Montgomery digit to 0 and to 2^W - 1; addends whose carry
    runs through every low limb into the top one."""
    K, N, p = F.K, F.N, F.P
    zero = [0] * N
    xb = 32 if F.name == "f29" else 512  # base coordinate x~ << SHIFT (f28: lazy words)
    neg = NEG_BASE[F.name]
    out = {k: [] for k in ("mul", "mul_add", "mul2_add", "mul2_add5", "sqr", "sqr_add")}

    def sites(v):
        """v(bound): an N-form value below bound p"""
        X, Y, ZZ, ZZZ = v(10), v(3), v(3), v(3)
        x2, y2 = v(xb), F.ksub(neg, v(1) if v is not top0 else zero)
        Pv, R, PP, PPP, Q, X3 = v(18), v(6), v(4), v(2), v(2), v(10)
        U, V, Wv, S, Mv = F.times(Y, 2), v(2), v(2), v(2), v(4)
        T = F.add_ksub(Q, K["K16"], X3 if v is not top0 else zero)
        neg_pq = F.ksub2(K["K8"], PPP if v is not top0 else zero, Q if v is not top0 else zero)
        out["mul_add"] += [(x2, ZZ, F.ksub(K["K16"], X)), (y2, ZZZ, F.ksub(K["K4"], Y)), (X, ZZ, F.ksub(K["K4"], PPP))]
        out["sqr"] += [(Pv,), (U,), (Mv,), (R,)]
        out["mul"] += [(Pv, PP), (X, PP), (U, V), (X, F.times(X, 3)), (V, ZZ), (ZZZ, PPP)]
        out["sqr_add"] += [(R, neg_pq), (Mv, F.ksub2(K["K8"], zero, S))]
        out["mul2_add"] += [(R, T, F.ksub(K["K4"], Y), PPP), (Mv, T, F.ksub(K["K4"], Wv), Y)]
        # lane pairs (component values a0, a1, b0, b1): lane 0 a0 b0 + a1 (K - b1), lane 1 a0 b1 + a1 b0
        a0, a1 = v(10), v(10)
        for Kn in ("K4", "K16") if F.name == "f29" else ("K4", "K8", "K32"):
            hi = {"K4": 3, "K8": 6, "K16": 10, "K32": 30}[Kn]  # the negated operand's bound at that site
            b0, b1 = v(hi), v(hi)
            out["mul2_add"] += [(a0, b0, a1, F.ksub(K[Kn], b1)), (a0, b1, a1, b0)]
        a0, a1 = v(3), v(3)
        nx = K["K33"] if F.name == "f29" else K["K16"]
        e = F.ksub(nx, v(32) if F.name == "f29" else X)
        out["mul2_add5"] += [(x2, ZZ, v(xb), F.ksub(K["K4"], ZZZ), e), (x2, ZZZ, v(xb), ZZ, e)]
        out["mul2_add5"] += [(a0, T, a1, F.ksub(K["K32R3"], T), F.ksub(K["K4"], Wv)), (a0, T, a1, T, F.ksub(K["K4"], Wv))]
        # the squares' operands: lane 0 (a0 + a1)(a0 + K - a1), lane 1 a0 (2 a1)
        for Kn in ("K4", "K8R1") if F.name == "f29" else ("K4", "K16", "K32"):
            hi = {"K4": 3, "K8R1": 6, "K16": 12, "K32": 18}[Kn]  # the squared value's bound at that site
            for c0, c1 in ((v(hi), v(hi)), (v(hi), zero), (zero, v(hi))):
                x, y = F.add(c0, c1), F.add(c0, F.ksub(K[Kn], c1))
                out["mul"] += [(x, y), (c0, F.times(c1, 2))]
                out["mul_add"] += [(x, y, neg_pq), (c0, F.times(c1, 2), neg_pq)]

    top0 = lambda b: ones(F, b)  # noqa: E731
    sites(top0)
    sites(lambda b: F.top_rep(rng.randrange(p), b))
    for _ in range(n_random):
        sites(lambda b: F.limbs(rng.randrange(b * p)))
    for k, n in (("mul", 2), ("mul_add", 3), ("mul2_add", 4), ("mul2_add5", 5), ("sqr", 1), ("sqr_add", 2)):
        out[k].append((zero,) * n)
    # every Montgomery digit 0, 2^W - 1, and alternating ends
    for _ in range(8):
        for target in (0, F.M, 1, F.M - 1):
            a, b, c, d = (F.limbs(rng.randrange(3 * p)) for _ in range(4))
            a[0] |= 1
            e = F.ksub(K["K16"], F.limbs(rng.randrange(10 * p)))
            out["mul"].append((a, F.force_digits(a, b, target)))
            out["mul_add"].append((a, F.force_digits(a, b, target), e))
            out["mul2_add"].append((a, F.force_digits(a, b, target, c, d), c, d))
            out["mul2_add5"].append((a, F.force_digits(a, b, target, c, d), c, d, e))
    # addends that carry through every low limb into the top one
    for _ in range(8):
        a, b, c, d = (F.limbs(rng.randrange(10 * p)) for _ in range(4))
        out["mul_add"].append((a, b, F.rippling_addend(F.product_exact(a, b))))
        out["mul2_add5"].append((a, b, c, d, F.rippling_addend(F.product_exact(a, b, c, d))))
        out["sqr_add"].append((a, F.rippling_addend(F.product_exact(a, a))))
    return out


def product_expected(F, op, operands):
    """limbs of the product op on one operand tuple (preconditions asserted)"""
    if op == "sqr":
        return F.product_case(operands[0], operands[0])
    if op == "sqr_add":
        return F.product_case(operands[0], operands[0], e=operands[1])
    if op in ("mul", "mul_add"):
        return F.product_case(operands[0], operands[1], e=operands[2] if op == "mul_add" else None)
    return F.product_case(*operands)


def random_product_cases(F, rng, n):
    """n operand sets (a, b, c, d, e) with limbs up to 30 bits, built inside the
    preconditions of every product op: a, c < 2^30 and b, d < 2^29 per limb
    (2 N products of < 2^59 and N digit products stay below 2^64; a alone may
    be squared: N products of < 2^60), e < 2^31, top limbs < 2^26 (the result's
    top limb stays far below 2^32)."""
    def lim(bits):
        return [rng.randrange(1 << bits) for _ in range(F.N - 1)] + [rng.randrange(1 << 26)]
    return [(lim(30), lim(29), lim(30), lim(29), lim(31)) for _ in range(n)]


# reduce_shl5 / reduce: (values below, every quotient below).  f29: x~ < 2^255 shifted by 5,
# every q; f28: N-form with a 32-bit top limb (below 2^396; q < 2^15.3), every q a load can
# produce (lazy words < 2p shifted by 8, negated bases below 257p: q < 512) and a sample of
# the rest; fr29: values below 2^264, every q
REDUCE_RANGE = {"f29": (1 << 260, 1 << 30), "f28": (1 << 396, 520), "fr29": (1 << 264, 1 << 30)}


def reduce_inputs(F, rng, vmax, every_q_below, n_random=300, n_mid=100):
    """Limbs for reduce_shl5 / reduce over [0, vmax): random values, the
    quotient boundaries v = q p + d (d in 0, 1, p - 1) for every q below
    every_q_below, a geometric sample of the q above it up to vmax / p with
    the largest ones, and values whose top two limbs sit on, just below and
    just above a float32 rounding midpoint."""
    p = F.P
    qmax = vmax // p
    qs = list(range(min(every_q_below, qmax + 1)))
    q = every_q_below
    while q <= qmax:
        qs += [q - 1, q, q + 1]
        q = q * 3 // 2 + rng.randrange(3)
    qs += [qmax - 2, qmax - 1, qmax] + [rng.randrange(qmax + 1) for _ in range(n_random)]
    vals = [q * p + d for q in sorted(set(q for q in qs if 0 <= q <= qmax)) for d in (0, 1, p - 1)]
    vals += [rng.randrange(vmax) for _ in range(n_random)] + [0, vmax - 1]
    low = F.W * (F.N - 2)
    for hi, lo in F.midpoint_tops(vmax, n_mid, rng):
        vals.append((hi << (low + F.W)) | (lo << low) | rng.randrange(1 << low))
    return [F.limbs(v) for v in vals if v < vmax]


def check_reduced(F, v_limbs, r_limbs):
    """the contract of reduce_shl5 / reduce / from32: same residue, N-form, below 3p"""
    v, r = F.value(v_limbs), F.value(r_limbs)
    assert F.n_form(r_limbs) and r < 3 * F.P and r % F.P == v % F.P and (v - r) % F.P == 0, (v_limbs, r_limbs)
    q = (v - r) // F.P
    assert v // F.P - 2 <= q <= v // F.P, (v_limbs, q)


# ---- lane-pair products at the operand bounds of their call sites ----
PAIR_KINDS = {"pmul": 0, "pmul_add": 1, "psqr": 2, "psqr_add": 3}
PAIR_K = {"K4": 0, "K8": 1, "K16": 2, "K32": 3, "K32R3": 4, "K8R1": 5}
# (kind, K, a, b, e) per instantiation in msm/pair29.h / pair28.h (madd, add, dbl).  a, b: a
# bound in units of p (an N-form value below it), "base" (a negated base, K - y~ << SHIFT),
# "T" (Q + 16p - X3); e: "negx" (the accumulator's K - X at madd's P), "negw" (4p - W),
# "negpq" (8p - PPP - 2Q)
PAIR_SITES = {
    "f29": [("pmul", "K4", 32, 3, None), ("pmul", "K16", 3, 10, None),
            ("pmul_add", "K4", 32, 3, "negx"), ("pmul_add", "K4", "base", 3, "negx"),
            ("pmul_add", "K32R3", 3, "T", "negw"),
            ("psqr", "K4", 3, None, None), ("psqr", "K8R1", 6, None, None), ("psqr_add", "K4", 3, None, "negpq")],
    "f28": [("pmul", "K4", 18, 3, None), ("pmul", "K8", 2, 6, None), ("pmul", "K32", 10, 30, None),
            ("pmul_add", "K4", 512, 3, "negx"), ("pmul_add", "K4", "base", 3, "negx"),
            ("pmul_add", "K32R3", 10, "T", "negw"),
            ("psqr", "K32", 18, None, None), ("psqr", "K16", 12, None, None),
            ("psqr_add", "K16", 10, None, "negpq"), ("psqr_add", "K4", 2, None, "negpq")],
}


def pair_product_cases(PM, rng, n_random):
    """{(kind, K): [(a, b, e)]}: lane-pair operands (c0 limbs, c1 limbs) for every
    product instantiation of the lane-pair point formulas, at the top of the
    bounds (all-ones low limbs, also with one component zero), at the largest
    representatives of random residues and at random values"""
    F = PM.F
    K, p = F.K, F.P
    zero = [0] * F.N
    nx = K["K33"] if F.name == "f29" else K["K16"]
    xin = PM.IN_BOUNDS[0]
    out = {}

    def build(spec, v, extreme):
        if spec is None:
            return None
        if spec == "base":
            return F.ksub(NEG_BASE[F.name], zero if extreme else v(1))
        if spec == "T":
            return F.add_ksub(v(2), K["K16"], zero if extreme else v(10))
        if spec == "negx":
            return F.ksub(nx, v(xin))
        if spec == "negw":
            return F.ksub(K["K4"], v(2))
        if spec == "negpq":
            return F.ksub2(K["K8"], zero if extreme else v(2), zero if extreme else v(2))
        return v(spec)

    gens = [(lambda b: ones(F, b), True), (lambda b: F.top_rep(rng.randrange(p), min(b, 64)), False)]
    gens += [(lambda b: F.limbs(rng.randrange(b * p)), False)] * n_random
    for kind, Kn, sa, sb, se in PAIR_SITES[F.name]:
        lst = out.setdefault((kind, Kn), [])
        for v, extreme in gens:
            pair = lambda s: None if s is None else (build(s, v, extreme), build(s, v, extreme))  # noqa: E731
            lst.append((pair(sa), pair(sb), pair(se)))
            if extreme:  # one component zero: the widest K - b1 and a0 + K - a1
                a, b, e = pair(sa), pair(sb), pair(se)
                lst.append(((a[0], zero), (b[0], zero) if b else None, e))
                lst.append(((zero, a[1]), (zero, b[1]) if b else None, e))
        lst.append(((zero, zero), (zero, zero) if sb is not None else None, (zero, zero) if se else None))
    return out


def pair_product_expected(PM, kind, Kn, a, b, e):
    K = PM.F.K[Kn]
    return PM.pmul(a, b, K, e) if kind in ("pmul", "pmul_add") else PM.psqr(a, K, e)
