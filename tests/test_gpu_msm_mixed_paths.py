"""MSM windows of two widths (MsmPlan::make_mixed, set_mixed_windows) on the
paths tests/test_gpu_msm_mixed_windows.py does not reach: bucket chains, every
variant bit, the layouts at the ends of the accepted range, host chunks, memory
divisions and several devices, the working-set estimate, the 2^26 default plan
and the refusals.  Every result is compared bytewise with the CPU oracle on the
same inputs (each oracle answer computed once per module), every run asserts
last_schedule()["mixed_windows"], and every context is reset in `finally`.

(a) Chains.  W = 40 (1,760 buckets in all: chain tables and every join level's
offsets built in-stream before the accumulation, kChainsInStream) and W = 23
(25,600 buckets: tables before the accumulation, offsets after, kChainsBefore)
at 2^14 and 2^17 points, and W = 23 at 2^19 with one repeated scalar, the
longest chain a test of this cost builds.  Each under variant 0 and under bit
21, the device-side comparison of chain_flags_kernel's flags with the
accumulation's.  kChainsAfter -- tables from the accumulation's own flags,
what the 2^26 default runs -- is reached under mixed keys only by the 2^26
tests of tests/test_gpu_full_size.py: it needs 2^21 accumulation threads or a
window group, and mixed widths refuse the groups.

(b) Variants.  window_sums runs the uniform code once per width class, so each
variant bit is run at W = 16 (one narrow window of 15 bits, fifteen of 16), 20
(12 / 13 bits), 28 (9 / 10 bits: the narrow class by the scan, the wide one by
segments) and 40 (6 / 7 bits: both by the scan).

(c) Layout extremes: W = 64 (one narrow window of 3 bits), 85 (3 bits, none
wide), 127 (2 bits, B = 2, one wide window: the most windows the layout takes).

(d) Splits: host chunks, memory divisions, three logical devices.

(e) The working-set estimate against the allocation, contract (a) and (b) of
tests/test_gpu_msm_memory.py (that file's R, imported).

(f) The default plan at 2^26 and the refusals of window groups.  No MSM runs
there: the refused combination would abort inside the library.
"""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_msm_mixed_windows import R as FR_MODULUS
from test_gpu_msm_mixed_windows import crafted_scalars, mont

pytestmark = pytest.mark.gpu

CURVE, SF = "bn254_g1", "bn254_fr"
OTHER_CURVES = ["bn254_g2", "bls12_381_g1", "bls12_381_g2"]
N_SMALL = 3001


def info(curve):
    from tachyon_amd._lib import CURVE_INFO
    return CURVE_INFO[curve]


def neg_point(curve, p: bytes) -> bytes:
    """-P of an affine point (y -> -y componentwise in the base field)."""
    fq = "bn254_fq" if curve.startswith("bn254") else "bls12_381_fq"
    half = len(p) // 2
    return p[:half] + O.field_op(fq, "neg", p[half:])


@pytest.fixture(scope="module")
def ctx():
    """One context per curve for the whole module."""
    from tachyon_amd.msm import VariableBaseMSMGpu
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = VariableBaseMSMGpu(curve)
        return made[curve]

    yield get
    for m in made.values():
        m.close()


def run_case(m, W, variant, bases, scalars, n=None):
    """One run under W mixed-width windows and `variant`: (result, schedule)."""
    m.set_mixed_windows(W)
    try:
        m.set_variant(variant)
        got = m.run(bases, scalars, n)
        sched = m.last_schedule()
        assert sched["mixed_windows"], (W, hex(variant))
    finally:
        m.set_variant(0)
        m.set_mixed_windows(0)
    return got, sched


# ---- (a) chains ----

CHAIN_KINDS = ["random", "one_scalar", "three_scalars", "small", "zero"]


@pytest.fixture(scope="module")
def chain_data():
    """(bases, scalars, oracle result) per (logn, kind), each computed once."""
    bases, cases = {}, {}

    def get(logn, kind):
        n = 1 << logn
        if logn not in bases:
            bases[logn] = O.gen_bases(CURVE, 60 + logn, n, 64).tobytes()
        if (logn, kind) not in cases:
            if kind == "random":
                sc = O.gen_scalars(SF, 60 + logn, n).tobytes()
            elif kind == "one_scalar":
                sc = O.gen_scalars(SF, 61 + logn, 1).tobytes() * n
            elif kind == "three_scalars":
                sc = (O.gen_scalars(SF, 62 + logn, 3).tobytes() * (n // 3 + 1))[:32 * n]
            elif kind == "small":  # digit-0-heavy: values i % 5, most digits the reserved key
                sc = mont(SF, [i % 5 for i in range(64)]) * (n // 64)
            else:
                sc = bytes(32 * n)
            want = O.msm(CURVE, bases[logn], sc)[0]
            if kind == "zero":
                assert want == bytes(64)  # the identity
            cases[(logn, kind)] = (sc, want)
        return (bases[logn],) + cases[(logn, kind)]

    return get


def check_chains(m, W, logn, kind, data):
    bases, scalars, want = data
    for variant in (0, 1 << 21):
        got, sched = run_case(m, W, variant, bases, scalars)
        assert got == want, (W, logn, kind, hex(variant))
        if variant:
            assert sched["chains_checked"], (W, logn, kind)


@pytest.mark.parametrize("kind", CHAIN_KINDS)
@pytest.mark.parametrize("logn", [14, 17])
@pytest.mark.parametrize("W", [40, 23])
def test_mixed_chains(ctx, chain_data, W, logn, kind):
    """Random scalars (short chains), one repeated scalar (one bucket per
    window: the longest chains), three repeated scalars (a few long chains
    among short ones), small scalars and an all-zero vector (the zero digits'
    reserved key is one run at the end of the sorted entries, across all
    windows; the all-zero result is the identity)."""
    check_chains(ctx(CURVE), W, logn, kind, chain_data(logn, kind))


def test_mixed_longest_chain(ctx, chain_data):
    """2^19 points under one scalar, W = 23: every window's entries in one bucket."""
    check_chains(ctx(CURVE), 23, 19, "one_scalar", chain_data(19, "one_scalar"))


# ---- (b) variants ----

@pytest.fixture(scope="module")
def small_inputs():
    """n = 3001 per curve: random; one base and scalar repeated (every madd after
    a bucket's first a doubling); P, -P alternating under one scalar and one
    identity base at the end (cancellations: the identity)."""
    made = {}

    def get(curve):
        if curve not in made:
            pb, sf = info(curve)
            n = N_SMALL
            bases = O.gen_bases(curve, 71, n, 40).tobytes()
            scalars = O.gen_scalars(sf, 71, n).tobytes()
            g1, s1 = bases[:pb], scalars[:32]
            pm = (g1 + neg_point(curve, g1)) * (n // 2) + bytes(pb)
            cases = {"random": (bases, scalars), "doublings": (g1 * n, s1 * n), "cancel": (pm, s1 * n)}
            made[curve] = {k: (b, s, O.msm(curve, b, s)[0]) for k, (b, s) in cases.items()}
            assert made[curve]["cancel"][2] == bytes(pb)
        return made[curve]

    return get


G1_VARIANTS = [0, 1, 3, 12, 16, 32, 48, 128, 256, 512, 768, 1024, 2048, 1024 | 2048, 4096, 4096 | 128, 8192,
               8192 | 4096, 16384, 131072, 262144, 262144 | (1 << 23), 524288, 1 << 25, 1 << 27]


@pytest.mark.parametrize("variant", G1_VARIANTS, ids=hex)
@pytest.mark.parametrize("W", [16, 20, 28, 40])
def test_mixed_variants(ctx, small_inputs, W, variant):
    """Accumulation chunks (bits 0-1), all windows as one group (12), onesweep
    tile shapes (4-5), the separate recode (7), scalars per thread (8-9),
    rocPRIM's histogram (10), 8-byte staging (11), window sums by trees (12),
    base prefetch (13, 17), the FIPS field (18) with two-level sums (23), the
    one-launch segment tree (19), 8-byte entry loads (25), and bit 27, which
    changes nothing under an explicit W."""
    for name, (bases, scalars, want) in small_inputs(CURVE).items():
        got, _ = run_case(ctx(CURVE), W, variant, bases, scalars)
        assert got == want, (W, hex(variant), name)


@pytest.mark.parametrize("n", [1, 7, 4097, 12289])
def test_mixed_entry_reads_odd_sizes(ctx, n):
    """The mixed counterpart of test_msm_entry_reads_odd_sizes: odd n (a lane's
    last LDS-staged chunk runs into the entry array's slack; the last 16-byte
    pair is cut), accumulation chunks 2 K and K / 2, 8-byte loads, W = 23."""
    bases = O.gen_bases(CURVE, 73, n, 16).tobytes()
    scalars = O.gen_scalars(SF, 73 + n, n).tobytes()
    want = O.msm(CURVE, bases, scalars)[0]
    for variant in (0, 1, 3, 1 << 25):
        got, _ = run_case(ctx(CURVE), 23, variant, bases, scalars)
        assert got == want, (n, hex(variant))


OTHER_VARIANTS = [(c, v) for c in OTHER_CURVES for v in (0, 32768, 1 << 20, 1 << 22, 1 << 23, 1 << 24)]
OTHER_VARIANTS.append(("bls12_381_g2", 65536 | (1 << 20)))


@pytest.mark.parametrize("curve,variant", OTHER_VARIANTS, ids=lambda x: x if isinstance(x, str) else hex(x))
@pytest.mark.parametrize("W", [16, 20])
def test_mixed_other_curves_variants(ctx, small_inputs, curve, W, variant):
    """The other accumulation and reduction kernels under mixed keys: BLS12-381
    W = 16 (16 bits, none wide) and 20 (12 / 13 bits, 16 wide), BN254 G2 W = 16
    (15 / 16) and 20 (12 / 13); the one-lane kernel (bit 15), the FIPS fields
    (20), the FIPS reductions (22), two-level (23) and two-pass (24) window
    sums, out-of-line products (16)."""
    for name, (bases, scalars, want) in small_inputs(curve).items():
        got, _ = run_case(ctx(curve), W, variant, bases, scalars)
        assert got == want, (curve, W, hex(variant), name)


# ---- (c) layout extremes ----

@pytest.fixture(scope="module")
def extreme_data():
    n_max = 4097
    bases = O.gen_bases(CURVE, 75, n_max, 64).tobytes()
    scalars = O.gen_scalars(SF, 75, n_max).tobytes()
    want = {n: O.msm(CURVE, bases[:64 * n], scalars[:32 * n])[0] for n in (1, 300, 4097)}
    return bases, scalars, want


@pytest.mark.parametrize("n", [1, 300, 4097])
@pytest.mark.parametrize("W", [64, 85, 127])
def test_mixed_layout_extremes(ctx, extreme_data, W, n):
    bases, scalars, want = extreme_data
    got, _ = run_case(ctx(CURVE), W, 0, bases[:64 * n], scalars[:32 * n])
    assert got == want[n], (W, n)


@pytest.mark.parametrize("W", [64, 85, 127])
def test_mixed_layout_extremes_crafted_scalars(ctx, W):
    """n = 1, so the result is s P and each scalar checks the recode alone:
    2^k and 2^k - 1 around every window boundary, carries out of every window,
    the largest top digit."""
    m = ctx(CURVE)
    P = O.gen_bases(CURVE, 77, 1, 1).tobytes()
    vals = crafted_scalars(CURVE, W)
    assert vals[0] == 0 and vals[-1] == FR_MODULUS[SF] - 1
    ss = mont(SF, vals)
    m.set_mixed_windows(W)
    try:
        for i, v in enumerate(vals):
            s = ss[32 * i:32 * i + 32]
            assert m.run(P, s) == O.msm(CURVE, P, s)[0], (W, hex(v))
            assert m.last_schedule()["mixed_windows"]
    finally:
        m.set_mixed_windows(0)


# ---- (d) splits ----

N_SPLIT = (1 << 18) + 77
W_SPLIT = 23


@pytest.fixture(scope="module")
def split_data():
    """Device-generated inputs, their host copies and the oracle's result."""
    torch = pytest.importorskip("torch")
    from tachyon_amd import msm as M
    n = N_SPLIT
    d_b = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    d_s = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    M.gen_bases(CURVE, 79, n, 512, d_b.data_ptr())
    M.gen_scalars(SF, 79, n, d_s.data_ptr())
    torch.cuda.synchronize()
    hb, hs = d_b.cpu().numpy(), d_s.cpu().numpy()
    yield d_b, d_s, hb, hs, O.msm_np(CURVE, hb, hs)
    del d_b, d_s
    torch.cuda.empty_cache()


def fresh(curve, W=0):
    """A context that holds nothing yet, as _fresh of test_gpu_msm_memory.py."""
    from tachyon_amd.msm import VariableBaseMSMGpu
    m = VariableBaseMSMGpu(curve)
    assert m.held_bytes() == 0
    if W:
        m.set_mixed_windows(W)
    return m


@pytest.mark.parametrize("chunks,on_host", [(3, "both"), (8, "bases"), (5, "scalars")])
def test_mixed_host_pipelined_chunks(split_data, chunks, on_host, monkeypatch):
    """run_host_pipelined: every chunk takes its own mixed plan and the chunks'
    window sums are combined by that plan's widths; the last chunk is shorter."""
    d_b, d_s, hb, hs, want = split_data
    monkeypatch.setenv("TACHYON_MSM_HOST_CHUNKS", str(chunks))
    b = d_b if on_host == "scalars" else hb
    s = d_s if on_host == "bases" else hs
    m = fresh(CURVE, W_SPLIT)
    try:
        assert m.run(b, s, N_SPLIT) == want
        assert m.last_schedule()["mixed_windows"]
        assert m.last_divisions() == chunks
    finally:
        m.set_mixed_windows(0)
        m.close()


@pytest.mark.parametrize("where", ["device", "host"])
def test_mixed_memory_divisions(split_data, where, monkeypatch):
    """TACHYON_MSM_MEM_LIMIT = run_bytes(n): 90 % of it is the budget, so the run
    no longer fits and is divided.  memory_divisions halves the chunk until it
    fits and throws (an abort through the C-ABI) once a chunk that does not fit
    is down to 2^16 points, so the same walk is made here first, on run_bytes,
    and the test fails before the library could reach that throw.

    The halves do not fit: run_bytes(262221) = 199042410, the budget is
    179138169 and run_bytes(131111) = 180402714, because the plan takes
    accumulation chunks of K = 16 entries up to 2^22 entries (3.0 M here) and
    K = 46 for the 6.0 M of the whole run, so the half has more accumulation
    threads (188 K against 131 K), each with its pieces and table rows.  The
    run is divided in four (65556 points each), which the walk predicts and
    the test asserts."""
    d_b, d_s, hb, hs, want = split_data
    n = N_SPLIT
    monkeypatch.delenv("TACHYON_MSM_HOST_CHUNKS", raising=False)
    m = fresh(CURVE, W_SPLIT)
    try:
        limit = m.run_bytes(n)
        budget = limit // 10 * 9
        # the uploaded inputs stay resident next to every chunk's working set
        resident = n * (64 + 32) if where == "host" else 0
        assert resident + m.run_bytes(n) > budget
        d = 1
        while resident + m.run_bytes((n + d - 1) // d) > budget:
            assert (n + d - 1) // d > 1 << 16, (d, budget)  # the library would throw here
            d *= 2
        assert d >= 2
        monkeypatch.setenv("TACHYON_MSM_MEM_LIMIT", str(limit))
        got = m.run(d_b, d_s, n) if where == "device" else m.run(hb, hs, n)
        assert got == want
        assert m.last_schedule()["mixed_windows"]
        assert m.last_divisions() == d >= 2
    finally:
        m.set_mixed_windows(0)
        m.close()


@pytest.mark.parametrize("mixed_first", [True, False])
def test_mixed_multi_device(mixed_first):
    """Three logical devices: set_mixed_windows before set_devices (copy_settings
    hands it to the new shards) and after (MsmMultiDevice::set_mixed_windows)."""
    n = 5001
    bases = O.gen_bases(CURVE, 81, n, 64).tobytes()
    scalars = O.gen_scalars(SF, 81, n).tobytes()
    want = O.msm(CURVE, bases, scalars)[0]
    m = fresh(CURVE)
    try:
        if mixed_first:
            m.set_mixed_windows(W_SPLIT)
            m.set_devices([0, 0, 0])
        else:
            m.set_devices([0, 0, 0])
            m.set_mixed_windows(W_SPLIT)
        assert m.run(bases, scalars) == want
        assert m.last_schedule()["mixed_windows"]
        shards = m.last_shards()
        assert [d for d, _, _ in shards] == [0, 0, 0] and sum(p for _, p, _ in shards) == n
        m.set_mixed_windows(0)  # reaches the shards too
        assert m.run(bases, scalars) == want
        assert not m.last_schedule()["mixed_windows"]
    finally:
        m.set_mixed_windows(0)
        m.set_devices([])
        m.close()


# ---- (e) the estimate ----

EST_NMAX = (1 << 17) + 5
EST_CASES = ([(CURVE, W, n) for W in (16, 20, 23, 28, 32, 40) for n in (300, 4097, 1 << 16, EST_NMAX)] +
             [(c, 20, n) for c in OTHER_CURVES for n in (4097, 1 << 16)])


@pytest.fixture(scope="module")
def est_inputs():
    """One device array of EST_NMAX bases / scalars per curve (prefixes are the
    cases) and the oracle's result per (curve, n), computed once."""
    torch = pytest.importorskip("torch")
    from tachyon_amd import msm as M
    dev, want = {}, {}

    def get(curve, n):
        pb, sf = info(curve)
        if curve not in dev:
            d_b = torch.empty(EST_NMAX * pb, dtype=torch.uint8, device="cuda")
            d_s = torch.empty(EST_NMAX * 32, dtype=torch.uint8, device="cuda")
            M.gen_bases(curve, 83, EST_NMAX, 512, d_b.data_ptr())
            M.gen_scalars(sf, 83, EST_NMAX, d_s.data_ptr())
            torch.cuda.synchronize()
            dev[curve] = (d_b, d_s, d_b.cpu().numpy(), d_s.cpu().numpy())
        d_b, d_s, hb, hs = dev[curve]
        if (curve, n) not in want:
            want[(curve, n)] = O.msm_np(curve, hb[:n * pb], hs[:n * 32])
        return d_b[:n * pb], d_s[:n * 32], want[(curve, n)]

    yield get
    dev.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("curve,W,n", EST_CASES)
def test_mixed_estimate_covers_allocation(est_inputs, curve, W, n):
    """One run on a fresh context.  (a) held_bytes() <= run_bytes(n), always.
    (b) run_bytes(n) <= R held_bytes() from 2^16 points, where the recode fed
    the sort: R was measured on that schedule, and rocPRIM's sort scratch (W =
    40, whose recode scatter passes 128 KiB of LDS) is estimated as another
    copy of the entries, which it does not reach."""
    from test_gpu_msm_memory import R, R_FROM
    d_b, d_s, want = est_inputs(curve, n)
    m = fresh(curve, W)
    try:
        est = m.run_bytes(n)
        got = m.run(d_b, d_s, n)
        sched = m.last_schedule()
        held = m.held_bytes()
        assert sched["mixed_windows"] and m.last_divisions() == 1
    finally:
        m.set_mixed_windows(0)
        m.close()
    print(f"MEM {curve} W={W} n={n} run_bytes={est} held_bytes={held} ratio={est / max(1, held):.4f} "
          f"short_by={max(0, held - est)} recode_fed_sort={sched['recode_fed_sort']}")
    assert got == want
    assert 0 < held <= est, (curve, W, n, held, est, held - est)  # (a)
    if n >= R_FROM and sched["recode_fed_sort"]:
        assert est <= R * held, (curve, W, n, est, held, est / held)  # (b)


# ---- (f) the default plan and the refusals (no MSM is run) ----

def test_default_plan_is_mixed_from_2_26(ctx):
    """BN254 G1 over 2^25 points: 12 windows of 21 and 22 bits; set_variant bit
    27 restores the 13 uniform windows of 20 bits; the other curves keep them."""
    from tachyon_amd import msm as M
    sizes = [1 << 26, (1 << 25) + 1, 1 << 25]
    m = ctx(CURVE)
    try:
        assert [m.plan_windows(n) for n in sizes] == [12, 12, 13]
        m.set_variant(1 << 27)
        assert [m.plan_windows(n) for n in sizes] == [13, 13, 13]
    finally:
        m.set_variant(0)
    assert [M.plan(CURVE, n) for n in sizes] == [(21, 12), (21, 12), (20, 13)]
    for curve in OTHER_CURVES:
        assert M.plan(curve, 1 << 26) == (20, 13), curve
        assert ctx(curve).plan_windows(1 << 26) == 13, curve


def test_mixed_refuses_window_groups(ctx):
    """One or two windows per sort group (set_variant bits 2-3 = 1, 2) are not a
    plain run: with mixed widths they are refused on either side, by the
    wrapper (ValueError naming both) and by the library (0), nothing changed.
    The combination is never run: run_windows would throw and the C-ABI abort."""
    from tachyon_amd._lib import lib
    m = ctx(CURVE)
    L = lib()
    n = 5000
    try:
        m.set_mixed_windows(23)
        before = (m.plan_windows(n), m.run_bytes(n))
        assert before[0] == 23
        for v in (4, 8, 4 | 1, 8 | 4096):
            with pytest.raises(ValueError, match="mixed-width windows"):
                m.set_variant(v)
            assert L.tachyon_mi355x_msm_gpu_set_variant(m.curve_id, m._ctx, v) == 0
            assert m.variant == 0 and (m.plan_windows(n), m.run_bytes(n)) == before, v
        m.set_variant(12)  # all windows in one group: the plain run's own grouping
        assert m.variant == 12 and m.plan_windows(n) == 23
        m.set_variant(0)
        m.set_mixed_windows(0)
        for v in (4, 8):
            m.set_variant(v)
            before = (m.plan_windows(n), m.run_bytes(n))
            with pytest.raises(ValueError, match="per sort group"):
                m.set_mixed_windows(23)
            assert L.tachyon_mi355x_msm_gpu_set_mixed_windows(m.curve_id, m._ctx, 23) == 0
            assert m.mixed_windows == 0 and (m.plan_windows(n), m.run_bytes(n)) == before, v
            m.set_mixed_windows(0)  # switching off is always accepted
        m.set_variant(12)
        m.set_mixed_windows(23)
        assert m.plan_windows(n) == 23
    finally:
        m.set_mixed_windows(0)
        m.set_variant(0)
