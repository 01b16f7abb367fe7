"""The host Poseidon2 and DuplexChallenger of the library
(tachyon_mi355x_baby_bear_duplex_challenger_*, tachyon_amd.fri.DuplexChallenger)
on a machine without a GPU: the reference's known answer, the permutation
against the goldens and poseidon2_ref, a scripted walk step for step against
fri_ref.DuplexChallenger, and the refusals.  Nothing here touches the GPU.

The permutation is reached through a rate-16 challenger: observing 16 words
duplexes at once, so the state afterwards is the permutation of those words.
There are no tolerances: every word is a canonical field element."""
import ctypes
import json
import os

import numpy as np
import pytest

import fri_ref as F
import poseidon2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tachyon_amd", "libtachyon_mi355x.so")
P = R.P
EXTERNALS = ["horizen", "plonky3"]


@pytest.fixture(scope="module", autouse=True)
def built():
    assert os.path.exists(LIB), "libtachyon_mi355x.so is built by build()"


def stored(x) -> bytes:
    return R.to_bytes(R.mont_words(np.asarray(x, dtype=np.uint64).reshape(-1)))


def canon(data: bytes) -> np.ndarray:
    return R.from_mont_words(R.from_bytes(data))


def host_permute(state, external) -> np.ndarray:
    """the library's host permutation of one canonical state"""
    from tachyon_amd.fri import DuplexChallenger
    ch = DuplexChallenger(external, 16)
    assert ch.observe(stored(state))
    st, inp, out = ch.state()
    assert inp == b"" and out == st            # the full buffer was duplexed at once
    return canon(st)


def same_state(ch, ref) -> bool:
    st, inp, out = ch.state()
    return ((canon(st) == ref.state).all() and list(canon(inp)) == ref.inp and list(canon(out)) == ref.out)


def test_reference_known_answer():
    """duplex_challenger_unittest.cc:44-56: Plonky3's matrix, rate 4, observe
    0..19, then 10 samples; poseidon2_ref with a rate-4 duplex gives the same"""
    from tachyon_amd.fri import DuplexChallenger
    want = [1091695522, 747772208, 1145639564, 1789312616, 567623980, 179016966, 125050365, 1725901131, 65962335,
            1086560956]
    ch = DuplexChallenger("plonky3", 4)
    assert ch.observe(stored(np.arange(20)))
    assert list(canon(ch.sample(10))) == want

    state, inp, out = np.zeros(16, dtype=np.uint64), [], []
    for v in range(20):
        inp.append(v)
        if len(inp) == 4:
            state[:4] = inp
            inp = []
            state = R.permute(state[None, :], "plonky3")[0]
            out = list(state)
    assert [int(out.pop()) for _ in range(10)] == want      # the fixture is reachable from the repo's own reference


def test_host_permutation_goldens():
    with open(os.path.join(ROOT, "tests", "golden", "poseidon2_baby_bear.json")) as f:
        gold = json.load(f)
    ref, rec = gold["reference"], gold["recorded"]
    assert list(host_permute(np.arange(16), "horizen")) == ref["horizen_permute_0_to_15"]
    got = host_permute(np.arange(16), "plonky3")
    assert list(got) == rec["plonky3_permute_0_to_15"]
    assert list(got[:4]) == ref["plonky3_permute_0_to_15_lanes_0_to_3"] and got[15] == ref["plonky3_permute_0_to_15_lane_15"]
    assert list(host_permute(np.full(16, P - 1), "horizen")) == rec["horizen_permute_all_p_minus_1"]


@pytest.mark.parametrize("external", EXTERNALS)
def test_host_permutation_against_poseidon2_ref(external):
    rng = np.random.default_rng(20250)
    states = rng.integers(0, P, size=(64, 16), dtype=np.uint64)
    states = np.concatenate([states, np.zeros((1, 16), dtype=np.uint64), np.full((1, 16), P - 1, dtype=np.uint64)])
    want = R.permute(states, external)
    for s, w in zip(states, want):
        assert (host_permute(s, external) == w).all()


@pytest.mark.parametrize("external", EXTERNALS)
def test_walk_against_fri_ref(external):
    """rate 8: the state and both buffers equal fri_ref's after every step"""
    from tachyon_amd.fri import DuplexChallenger
    ch, ref = DuplexChallenger(external, 8), F.DuplexChallenger(external)
    rng = np.random.default_rng(77)
    assert same_state(ch, ref)

    def observe(n):
        v = rng.integers(0, P, size=n, dtype=np.uint64)
        assert ch.observe(stored(v))
        ref.observe(v)
        assert same_state(ch, ref)

    def sample():
        got = int(canon(ch.sample())[0])
        assert got == ref.sample() and same_state(ch, ref)

    observe(3)                       # a partial observe
    sample()                         # duplexes the three words
    observe(8)                       # fills the rate: the duplex happens at once
    assert ch.state()[1] == b"" and len(ch.state()[2]) == 64
    for _ in range(18):              # the output buffer runs out after 16 and is refilled
        sample()
    observe(1)                       # an observe after a sample clears the outputs
    assert ch.state()[2] == b""
    assert (canon(ch.sample_ext()) == ref.sample_ext()).all() and same_state(ch, ref)
    for bits in (0, 1, 27, 30):
        assert ch.sample_bits(bits) == ref.sample_bits(bits) and same_state(ch, ref)
    observe(5)
    for bits, witness in ((0, 12345), (4, 7), (4, P - 1)):
        w = int(R.mont_words([witness])[0])
        assert ch.check_witness(bits, w) == ref.check_witness(bits, witness) and same_state(ch, ref)
    # a witness that passes: fri_ref's own grind, on a clone
    good = ref.clone().grind(6)
    assert ch.check_witness(6, int(R.mont_words([good])[0])) and ref.check_witness(6, good) and same_state(ch, ref)

    # clone independence
    twin, ref_twin = ch.clone(), ref.clone()
    assert same_state(twin, ref_twin)
    assert twin.observe(stored([1, 2, 3]))
    ref_twin.observe([1, 2, 3])
    assert same_state(twin, ref_twin) and same_state(ch, ref)
    sample()
    assert same_state(twin, ref_twin)
    assert int(canon(twin.sample())[0]) == ref_twin.sample() and same_state(ch, ref)


def test_refusals():
    from tachyon_amd._lib import lib
    from tachyon_amd.fri import DuplexChallenger
    L = lib()
    create = L.tachyon_mi355x_baby_bear_duplex_challenger_create
    for ext_id, rate in [(0, 0), (0, 17), (2, 8), (-1, 8)]:
        assert not create(ext_id, rate)
    for rate in (1, 16):
        h = create(1, rate)
        assert h
        L.tachyon_mi355x_baby_bear_duplex_challenger_destroy(h)
    ch, ref = DuplexChallenger("horizen", 8), F.DuplexChallenger("horizen")
    assert ch.observe(stored([5, 6]))
    ref.observe([5, 6])
    before = ch.state()
    # a word >= p anywhere in the batch: nothing is observed
    assert not ch.observe(stored([1, 2]) + (P).to_bytes(4, "little"))
    assert not ch.observe(b"\xff\xff\xff\xff")
    assert ch.sample_bits(31) is None and ch.sample_bits(32) is None
    assert not ch.check_witness(31, 1) and not ch.check_witness(4, P)
    assert ch.state() == before and same_state(ch, ref)
    out = ctypes.c_uint32()
    assert L.tachyon_mi355x_baby_bear_duplex_challenger_observe(None, None, 0) == 0
    assert L.tachyon_mi355x_baby_bear_duplex_challenger_observe(ch._h, None, 1) == 0
    assert L.tachyon_mi355x_baby_bear_duplex_challenger_sample(ch._h, None, 1) == 0
    assert L.tachyon_mi355x_baby_bear_duplex_challenger_sample_ext(ch._h, None) == 0
    assert L.tachyon_mi355x_baby_bear_duplex_challenger_sample_bits(ch._h, 3, None) == 0
    assert L.tachyon_mi355x_baby_bear_duplex_challenger_sample_bits(None, 3, ctypes.byref(out)) == 0
    assert L.tachyon_mi355x_baby_bear_duplex_challenger_state(ch._h, None) == 0
    assert not L.tachyon_mi355x_baby_bear_duplex_challenger_clone(None)
    # grinding refuses its arguments before it looks for a GPU
    assert ch.grind(31) is None and ch.grind_range(4, 5, 5) is None and ch.grind_range(4, 0, P + 1) is None
    assert ch.state() == before
    assert int(canon(ch.sample())[0]) == ref.sample()       # and the transcript goes on
