"""BN254 G1's window sums in one pass over the windows of both widths
(window_sums29: window_segment29_kernel over the concatenated bucket array,
reduce_uniform29_kernel levels and window_tree29_kernel over all windows).

Every result is compared bytewise with the CPU oracle on the same inputs; the
random input and its oracle answer are computed once per module.  n is 4096 at
most: the window sums depend on the layout (set_mixed_windows /
set_window_bits) and on the segment length L (set_window_segment), not on n.

With kBlock = 256 threads and B the buckets of a narrow window (2 B in a wide
one), S = B / L segment sums per narrow window:
 * a class with <= 256 buckets per window goes by window_scan29, the others by
   segments; binary levels run while the widest window of the pass has more
   than 256 sums, then one tree launch;
 * the rule's L is MsmPlan::seg_for over all the buckets nb of the pass (2
   below 196,608 buckets, doubling with nb up to 64 from 3,145,728) and doubles
   on while nb / L threads exceed one resident round of the kernel, so the
   layouts W = 20, 17, 16, 15, 14, 13, 12 (nb = 71,680 .. 15,728,640) take
   L = 2, 4, 8, 16, 32, 64 and 128 at any n; set_window_segment forces every
   power of two from 2 to 256.
"""
import random

import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

CURVE, SF = "bn254_g1", "bn254_fr"
FR = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
N = 4096
LENGTHS = [2, 4, 8, 16, 32, 64, 128, 256]


def mont(values):
    return O.field_op(SF, "to_mont", b"".join(v.to_bytes(32, "little") for v in values))


@pytest.fixture(scope="module")
def m():
    from tachyon_amd.msm import VariableBaseMSMGpu
    ctx = VariableBaseMSMGpu(CURVE)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def data():
    """N bases, N random scalars and the oracle's answer, computed once."""
    bases = O.gen_bases(CURVE, 91, N, 64).tobytes()
    scalars = O.gen_scalars(SF, 91, N).tobytes()
    return bases, scalars, O.msm(CURVE, bases, scalars)[0]


def run(m, bases, scalars, W=0, c=0, L=0):
    """One run under W mixed-width windows (or c forced window bits) and segment length L."""
    try:
        if c:
            m.set_window_bits(c)
        if W:
            m.set_mixed_windows(W)
        m.set_window_segment(L)
        got = m.run(bases, scalars)
        assert m.last_schedule()["mixed_windows"] == bool(W), (W, c, L)
    finally:
        m.set_window_segment(0)
        m.set_mixed_windows(0)
        m.set_window_bits(0)
    return got


def layout(W):
    """(bit offsets, widths, narrow) of W mixed-width windows."""
    from tachyon_amd import msm as M
    lay = M.mixed_layout(CURVE, W)
    boff = lay["bit_offsets"]
    return boff, [boff[w + 1] - boff[w] for w in range(W)], W - lay["n_wide"]


# W: 17 none wide (15 bits); 127 one wide window (2 and 3 bits, both classes by the scan); 64 one narrow window (3
# and 4 bits, scans); 40 both by the scan (6 / 7 bits); 28 the narrow class by the scan (256 buckets), the three
# wide windows by segments; 20 (12 / 13 bits) and 16 (one narrow window of 15 bits) both by segments
@pytest.mark.parametrize("W", [17, 127, 64, 40, 28, 20, 16, 15, 14, 13, 12])
def test_mixed_layouts_rule_length(m, data, W):
    """Both classes non-empty, a class empty, a class of one window, a class
    the segment pass does not own, and every L the rule chooses (module text)."""
    bases, scalars, want = data
    assert run(m, bases, scalars, W=W) == want, W


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("W", [20, 17, 28])
def test_mixed_every_length(m, data, W, L):
    """W = 20 (B = 2048): L = 16 leaves 128 / 256 sums per window, the tree
    launch alone; L = 8 leaves 256 / 512, one binary level first; L = 2 three
    levels.  W = 17 (B = 16384, none wide): L = 64 -> S = 256 tree alone, L = 32
    one level.  W = 28: the wide windows (512 buckets) by segments -- L = 2
    -> 256 sums, the tree alone; L = 256 is cut to the narrow window's 256
    buckets, two sums -- beside the narrow class's scan."""
    bases, scalars, want = data
    assert run(m, bases, scalars, W=W, L=L) == want, (W, L)


@pytest.mark.parametrize("logn", [10, 14, 16])
def test_uniform_default_sizes(m, logn):
    """The uniform default plans of 2^10, 2^14 and 2^16 points."""
    n = 1 << logn
    bases = O.gen_bases(CURVE, 92, n, 64).tobytes()
    scalars = O.gen_scalars(SF, 92, n).tobytes()
    assert run(m, bases, scalars) == O.msm(CURVE, bases, scalars)[0], logn


@pytest.mark.parametrize("L", [0] + LENGTHS)
@pytest.mark.parametrize("c", [10, 13])
def test_uniform_segments(m, data, c, L):
    """The uniform plan through the same kernels (narrow = W).  c = 13 (B =
    4096): L = 16 -> S = 256, the tree launch alone; L = 8 -> 512, one level
    first.  c = 10 (B = 512): L = 2 -> S = 256; L = 256 -> two sums."""
    bases, scalars, want = data
    assert run(m, bases, scalars, c=c, L=L) == want, (c, L)


def edge_scalars(W):
    """{name: scalars} that put the weight on the fix-up's edges under W windows."""
    boff, width, narrow = layout(W)
    top = W - 1
    cases = {}
    # digit 1 in every window: the first bucket of segment 0 (j L = 0)
    cases["first_bucket"] = [sum(1 << boff[w] for w in range(W))]
    # the largest digit the top window reaches below r (unsigned, carry folded in): the largest j L of the top window
    cases["top_digit"] = [(FR >> boff[top]) << boff[top], ((FR >> boff[top]) << boff[top]) - 1]
    # raw 2^(width - 1): digit -2^(width - 1), the LAST bucket of the last segment, and a carry of 1 into the window
    # above, its first bucket -- in the last window below the top (a wide one where two are wide: the largest j L
    # there is), and at the seam narrow - 1 | narrow of the concatenated array
    cases["last_bucket"] = [1 << (boff[top] - 1)]
    if 0 < narrow < W:
        cases["seam"] = [1 << (boff[narrow] - 1), (1 << (boff[narrow] - 1)) + (1 << boff[narrow - 1])]
    # the last bucket of every window below the top at once
    cases["all_last"] = [sum(1 << (boff[w + 1] - 1) for w in range(W - 1))]
    return cases


def odd_digit_scalars(W, count, seed):
    """Scalars whose digits are odd in every window (no carries: below half the
    window): every other bucket stays empty, identity loads in the running sums."""
    boff, width, _ = layout(W)
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        v = 0
        for w in range(W):
            half = 1 << (width[w] - 1)
            hi = min(half, FR >> boff[w]) if w == W - 1 else half
            v += (rng.randrange(0, max(1, (hi - 1) // 2)) * 2 + 1) << boff[w]
        assert v < FR
        out.append(v)
    return out


@pytest.mark.parametrize("L", [0, 2, 16, 128])
@pytest.mark.parametrize("W", [20, 28, 16])
def test_fixup_edges(m, data, W, L):
    """The (j L) R fix-up at its edges (edge_scalars), three points per scalar."""
    bases = data[0]
    for name, vals in edge_scalars(W).items():
        sc = mont([v for v in vals for _ in range(3)])
        b = bases[:64 * 3 * len(vals)]
        assert run(m, b, sc, W=W, L=L) == O.msm(CURVE, b, sc)[0], (W, L, name)


@pytest.mark.parametrize("W,L", [(20, 0), (20, 16), (28, 0), (28, 4), (17, 64)])
def test_every_other_bucket_empty(m, data, W, L):
    bases = data[0]
    sc = mont(odd_digit_scalars(W, N, 7 * W))
    assert run(m, bases, sc, W=W, L=L) == O.msm(CURVE, bases, sc)[0], (W, L)


def test_bls12_381_g1_untouched():
    """BLS12-381 G1 keeps its per-class reduction: uniform and 20 mixed windows."""
    from tachyon_amd.msm import VariableBaseMSMGpu
    n = 3001
    bases = O.gen_bases("bls12_381_g1", 93, n, 40).tobytes()
    scalars = O.gen_scalars("bls12_381_fr", 93, n).tobytes()
    want = O.msm("bls12_381_g1", bases, scalars)[0]
    ctx = VariableBaseMSMGpu("bls12_381_g1")
    try:
        assert ctx.run(bases, scalars) == want
        ctx.set_mixed_windows(20)
        assert ctx.run(bases, scalars) == want
    finally:
        ctx.set_mixed_windows(0)
        ctx.close()


def test_segment_length_refused(m):
    for bad in (1, 3, 48, 512):
        with pytest.raises(ValueError):
            m.set_window_segment(bad)
