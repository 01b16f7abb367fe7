"""MSM windows of two widths (MsmPlan::make_mixed, set_mixed_windows): W windows
of c_lo = (bits + 1) // W bits, the top bits + 1 - W c_lo of them one bit wider,
sort keys = bucket indices.  Every comparison is bytewise on the affine result:
against the CPU oracle and against the same context under the uniform plan.

W = 40 (6 and 7 bits, 1,760 buckets: the rocPRIM sort, in-stream chains, scan
window sums), W = 23 (11 and 12 bits: fused recode, segment sums), W = 17
(15 bits, no wide window: must equal set_window_bits(15)) and W = 12 (21 and 22
bits, 15.7 M buckets: the layout BN254 G1 runs from 2^26 points).

The wide windows are the top ones, so the layout has one boundary, narrow below
wide; the crafted scalars put their edge digits on both sides of it.  A top
digit of 2^(c_top - 1) needs the top window's bits all set, i.e. a scalar of at
least 2^bits - 2^off_top > r: canonical scalars cannot reach it, so the largest
top digit a scalar below r gives (r's top bits, the carry folded in) stands for
it."""
import numpy as np
import pytest

from oracle import oracle as O

CURVE, SF = "bn254_g1", "bn254_fr"
BITS = {"bn254_g1": 254, "bn254_g2": 254, "bls12_381_g1": 255, "bls12_381_g2": 255}
R = {"bn254_fr": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
     "bls12_381_fr": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
WS = (40, 23, 17, 12)
NS = (1, 2, 3, 65, 300, 4096)
N_MAX = 4096


def expected_layout(bits, W):
    """The layout's arithmetic, restated: (c_lo, n_wide, widths low to high, total buckets)."""
    c_lo = (bits + 1) // W
    n_wide = bits + 1 - W * c_lo
    widths = [c_lo] * (W - n_wide) + [c_lo + 1] * n_wide
    return c_lo, n_wide, widths, sum(1 << (c - 1) for c in widths)


@pytest.mark.parametrize("curve", ["bn254_g1", "bls12_381_g1"])
def test_mixed_plan_arithmetic(curve):
    """The plan through the C entry point, W = 8 .. bits + 1, for 254- and
    255-bit scalars: the widths add up to bits + 1, the bit and bucket offsets
    are the running sums of the widths and of 2^(c_w - 1), the largest key is
    below the reserved key 2^key_bits - 1, and a layout over 24 key bits or
    with windows of one bit (W over (bits + 1) / 2) is refused."""
    from tachyon_amd import msm as M
    bits = BITS[curve]
    seen_ok = seen_refused = 0
    for W in range(8, bits + 2):
        c_lo, n_wide, widths, total = expected_layout(bits, W)
        lay = M.mixed_layout(curve, W)
        # the largest bucket index would reach the reserved 24-bit key, or the narrow windows have one bit
        if total - 1 >= (1 << 24) - 1 or c_lo < 2:
            assert lay is None, (W, lay)
            seen_refused += 1
            continue
        seen_ok += 1
        assert lay is not None, W
        assert (lay["c_lo"], lay["n_wide"]) == (c_lo, n_wide), (W, lay)
        boff, koff = lay["bit_offsets"], lay["bucket_offsets"]
        assert boff[0] == 0 and koff[0] == 0 and boff[W] == bits + 1 and koff[W] == total, (W, lay)
        assert [boff[w + 1] - boff[w] for w in range(W)] == widths, (W, lay)
        assert [koff[w + 1] - koff[w] for w in range(W)] == [1 << (c - 1) for c in widths], (W, lay)
        assert lay["key_bits"] <= 24 and koff[W] - 1 < (1 << lay["key_bits"]) - 1, (W, lay)
    assert seen_ok and seen_refused
    if bits == 254:  # nine windows of 21 bits and three of 22: 15,728,640 buckets; 11 windows need 26 key bits
        lay = M.mixed_layout(curve, 12)
        assert (lay["c_lo"], lay["n_wide"], lay["bucket_offsets"][12]) == (21, 3, 15728640)
        assert M.mixed_layout(curve, 11) is None
    else:  # 256 = 12 x 21 + 4: exactly 2^24 buckets, one too many
        assert M.mixed_layout(curve, 12) is None and M.mixed_layout(curve, 13) is not None


# ---- GPU ----

@pytest.fixture(scope="module")
def m():
    from tachyon_amd.msm import VariableBaseMSMGpu
    ctx = VariableBaseMSMGpu(CURVE)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def data():
    """One input for every size (prefixes) and the oracle's results, computed once."""
    bases = O.gen_bases(CURVE, 41, N_MAX, 64).tobytes()
    scalars = O.gen_scalars(SF, 41, N_MAX).tobytes()
    expect = {n: O.msm(CURVE, bases[:64 * n], scalars[:32 * n])[0] for n in NS}
    return bases, scalars, expect


def run_mixed(m, W, bases, scalars):
    m.set_mixed_windows(W)
    try:
        got = m.run(bases, scalars)
        assert m.last_schedule()["mixed_windows"], W
    finally:
        m.set_mixed_windows(0)
    return got


def mont(sf, values):
    return O.field_op(sf, "to_mont", b"".join(v.to_bytes(32, "little") for v in values))


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("W", WS)
def test_mixed_vs_oracle_and_uniform(m, data, W, n):
    bases, scalars, expect = data
    b, s = bases[:64 * n], scalars[:32 * n]
    got = run_mixed(m, W, b, s)
    assert got == expect[n], (W, n)
    uniform = m.run(b, s)
    assert not m.last_schedule()["mixed_windows"]
    assert got == uniform, (W, n)
    if W == 17:  # no wide window: the same windows as uniform c = 15
        m.set_window_bits(15)
        try:
            assert got == m.run(b, s)
        finally:
            m.set_window_bits(0)


def crafted_scalars(curve, W):
    from tachyon_amd import msm as M
    lay = M.mixed_layout(curve, W)
    r = R[SF]
    boff = lay["bit_offsets"]
    narrow = W - lay["n_wide"]
    vals = {0, 1, r - 1}
    for k0 in boff:  # 2^k and 2^k - 1 at every window boundary and one either side
        for k in (k0 - 1, k0, k0 + 1):
            if 0 <= k and (1 << k) < r:
                vals |= {1 << k, (1 << k) - 1}
    # a digit of exactly -2^(c_w - 1) (raw 2^(c_w - 1), carry out) in the windows on
    # both sides of the narrow -> wide boundary, alone and together
    sides = [w for w in (narrow - 1, narrow) if 0 <= w < W - 1]
    halves = [1 << (boff[w + 1] - 1) for w in sides]
    vals |= set(halves) | {sum(halves)}
    # the raw half in every window below the top: a carry out of every one of them
    vals.add(sum(1 << (boff[w + 1] - 1) for w in range(W - 1)))
    # the largest top digit a scalar below r reaches: r's top bits, every lower bit set (carry folded in)
    top = boff[W - 1]
    vals.add(((r >> top) << top) - 1)
    return sorted(v for v in vals if v < r)


@pytest.mark.gpu
@pytest.mark.parametrize("W", WS)
def test_mixed_recode_crafted_scalars(m, W):
    """n = 1: the result is s P, so each scalar checks the recode alone."""
    P = O.gen_bases(CURVE, 43, 1, 1).tobytes()
    vals = crafted_scalars(CURVE, W)
    ss = mont(SF, vals)
    m.set_mixed_windows(W)
    try:
        for i, v in enumerate(vals):
            s = ss[32 * i:32 * i + 32]
            assert m.run(P, s) == O.msm(CURVE, P, s)[0], (W, hex(v))
    finally:
        m.set_mixed_windows(0)


@pytest.mark.gpu
@pytest.mark.parametrize("W", (40, 12))
def test_mixed_edge_bases(m, data, W):
    """n = 4096: identity bases mixed in; one point repeated with one scalar
    (every madd after a bucket's first is P = acc, a doubling, and the bucket
    runs over many threads); P, -P pairs in one bucket (cancellations)."""
    bases, scalars, _ = data
    n = N_MAX
    arr = np.frombuffer(bases, dtype=np.uint8).reshape(n, 64).copy()
    arr[::7] = 0  # (0, 0) = the identity
    holes = arr.tobytes()
    assert run_mixed(m, W, holes, scalars) == O.msm(CURVE, holes, scalars)[0]
    g1, s1 = bases[:64], scalars[:32]
    assert run_mixed(m, W, g1 * n, s1 * n) == O.msm(CURVE, g1 * n, s1 * n)[0]
    neg = O.field_op("bn254_fq", "neg", g1[32:64])
    pm = (g1 + g1[:32] + neg) * (n // 2)
    assert run_mixed(m, W, pm, s1 * n) == bytes(64)


@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["bn254_g2", "bls12_381_g1", "bls12_381_g2"])
def test_mixed_other_curves(curve):
    """The other accumulation kernels decode the same keys: W = 20 over 254-bit
    (12 and 13 bits) and 255-bit (12 and 13 bits, 16 wide) scalars, n = 300."""
    from tachyon_amd._lib import CURVE_INFO
    from tachyon_amd.msm import VariableBaseMSMGpu
    pb, sf = CURVE_INFO[curve]
    n = 300
    bases = O.gen_bases(curve, 47, n, 16).tobytes()
    scalars = O.gen_scalars(sf, 47, n).tobytes()
    ctx = VariableBaseMSMGpu(curve)
    try:
        got = run_mixed(ctx, 20, bases, scalars)
        assert got == O.msm(curve, bases, scalars)[0]
        assert got == ctx.run(bases, scalars)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_mixed_refuses_other_modes(m, data):
    """Mixed widths are for a plain run: together with a batch, a fold, a window
    range or forced window bits they are an error, and so is a refused layout."""
    import torch
    bases, scalars, expect = data
    n = 64
    d_b = torch.frombuffer(bytearray(bases[:64 * n]), dtype=torch.uint8).cuda()
    d_s = torch.frombuffer(bytearray(scalars[:32 * n]), dtype=torch.uint8).cuda()
    d_out = torch.empty(2 * 64 * n, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        m.set_mixed_windows(11)  # 26 key bits
    assert m.mixed_windows == 0
    m.set_window_bits(10)
    try:
        with pytest.raises(ValueError):
            m.set_mixed_windows(40)
    finally:
        m.set_window_bits(0)
    m.set_mixed_windows(40)
    try:
        with pytest.raises(ValueError):
            m.set_window_bits(10)
        with pytest.raises(ValueError):
            m.run_batch(d_b, d_s, n // 2, 2)
        with pytest.raises(ValueError):
            m.fold_bases(d_b, n, 2, d_out)
        with pytest.raises(ValueError):
            m.run_folded(d_out, d_s, n, 2)
        with pytest.raises(ValueError):
            m.run_window_range(bases[:64 * n], scalars[:32 * n], 0, 3)
        # the library's own refusals, under the wrapper's
        from tachyon_amd._lib import lib
        out = torch.empty(2 * 64, dtype=torch.uint8).numpy()
        assert not lib().tachyon_mi355x_msm_gpu_batch_affine(m.curve_id, m._ctx, d_b.data_ptr(), n // 2, d_s.data_ptr(), 2,
                                                            out.ctypes.data)
        assert not lib().tachyon_mi355x_msm_gpu_fold_bases(m.curve_id, m._ctx, d_b.data_ptr(), n, 2, d_out.data_ptr())
        assert not lib().tachyon_mi355x_msm_gpu_folded_affine(m.curve_id, m._ctx, d_out.data_ptr(), d_s.data_ptr(), n, 2,
                                                             out.ctypes.data)
        # still a working context: the plain run under the mixed plan
        assert m.run(bases[:64 * 65], scalars[:32 * 65]) == expect[65]
        assert m.last_schedule()["mixed_windows"]
    finally:
        m.set_mixed_windows(0)
    assert m.run(bases[:64 * 65], scalars[:32 * 65]) == expect[65]
    assert not m.last_schedule()["mixed_windows"]
