"""The circom zkey / wtns readers (csrc/groth16/circom_parse.h) on the host
alone: check/circom_io_check.cc, a stand-alone program with its own main, built
under the address and undefined-behaviour sanitizers with nothing preloaded.
Runs without a GPU (the C-ABI aborts on a malformed file by design, so none of
this may go through it on a GPU machine).

This module writes the files (oracle.circom_format plus byte patches); the
program reads them and prints one verdict per file -- "parsed" with a dump,
"refused: circom: ..." (the readers' own refusal) or "error: ..." (any other
exception; a bare STL message is not a refusal, and a sanitizer report or a
crash loses the verdict line altogether).  A dump is compared with
oracle.circom_format: the three header counts, every point section byte for
byte, every coefficient as (matrix, constraint, signal, canonical value).

A refusal whose patched count is >= 2^24 must also be cheap: the child's peak
RSS (os.wait4) stays within 64 MiB of a valid parse's.  Before the readers
compared count x element size with the bytes left in the section, the smallest
such patch (num_vars = 2^26) took 4.1 GB and domain_size = 2^31 ended in the
sanitizer's out-of-memory abort.
"""
import os
import struct
import subprocess
import sys

import pytest

from oracle import circom_format as CF
from tachyon_amd import params as P

sys.path.insert(0, os.path.dirname(__file__))
from groth16_synth import synth_zkey  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tachyon_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
RSS_CAP_KIB = 64 * 1024  # over the valid file's peak: a cap, not a tuning number
R_OF = {"bn254": P.BN254_FR, "bls12_381": P.BLS12_381_FR}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("circom_io_check") / "circom_io_check"
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                        "-I" + os.path.join(CSRC, "field"), "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", str(out),
                        os.path.join(CSRC, "check", "circom_io_check.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


@pytest.fixture(scope="module")
def key3():
    """The synthetic BN254 key at log_n = 3 and its witness file."""
    z, full = synth_zkey("bn254", log_n=3, seed=31)
    return z, CF.write_wtns(full, P.BN254_FR)


# ---- running the program -------------------------------------------------

def run(exe, args, tmp_path):
    """(exit code, stdout, stderr, peak RSS in KiB) of one child."""
    out_p, err_p = tmp_path / "check.out", tmp_path / "check.err"
    with open(out_p, "wb") as fo, open(err_p, "wb") as fe:
        p = subprocess.Popen([exe] + [str(a) for a in args], stdout=fo, stderr=fe)
        _, status, ru = os.wait4(p.pid, 0)
        p.returncode = os.waitstatus_to_exitcode(status)
    return p.returncode, out_p.read_text(), err_p.read_text(), ru.ru_maxrss


def own_peak(stdout):
    """The child's own report of its peak resident set (KiB)."""
    last = stdout.splitlines()[-1].split()
    assert last[0] == "peak_rss_kib" and int(last[1]) > 0, stdout[-500:]
    return int(last[1])


def records(stdout):
    """[(path, verdict, {name: rest of the line | list for coef})] of a zkey / wtns run."""
    recs, cur = [], None
    for line in stdout.splitlines():
        if line.startswith("file "):
            cur = [line[5:], None, {"coef": []}]
        elif cur is not None and cur[1] is None:
            cur[1] = line
        elif line == "end":
            recs.append(tuple(cur))
            cur = None
        elif cur is not None:
            name, _, rest = line.partition(" ")
            if name == "coef":
                cur[2]["coef"].append(rest.split())
            else:
                cur[2][name] = rest.strip()
    assert cur is None, "the output ends inside a record:\n" + stdout[-2000:]
    return recs


def read_files(exe, kind, curve, blobs, tmp_path):
    """Runs the program over `blobs` ({name: bytes}) in one process; {name: (verdict, fields)}."""
    paths = []
    for name, data in blobs.items():
        p = tmp_path / name
        p.write_bytes(data)
        paths.append(p)
    code, out, err, _ = run(exe, [kind, curve] + paths, tmp_path)
    recs = records(out)
    assert len(recs) == len(blobs), (code, out[-2000:], err[-4000:])
    got = {os.path.basename(path): (verdict, fields) for path, verdict, fields in recs}
    assert code == (1 if any(v.startswith("error") for v, _ in got.values()) else 0), err[-4000:]
    return got


# ---- writing and patching files ------------------------------------------

def split_sections(data):
    """[(type, body)] in file order (repeated types kept)."""
    (count,) = struct.unpack_from("<I", data, 8)
    off, out = 12, []
    for _ in range(count):
        typ, size = struct.unpack_from("<IQ", data, off)
        out.append((typ, bytes(data[off + 12:off + 12 + size])))
        off += 12 + size
    return out


def join_sections(magic, version, sections):
    out = [magic, struct.pack("<II", version, len(sections))]
    for typ, body in sections:
        out += [struct.pack("<IQ", typ, len(body)), body]
    return b"".join(out)


def patch(data, off, new):
    return data[:off] + new + data[off + len(new):]


def u32(x):
    return struct.pack("<I", x)


def zkey_offsets(data):
    """File offsets of the fields the patches aim at."""
    secs = CF._sections(data, 8)
    g = secs[2][0]
    (n8q,) = struct.unpack_from("<I", data, g)
    (n8r,) = struct.unpack_from("<I", data, g + 4 + n8q)
    counts = g + 4 + n8q + 4 + n8r
    return dict(secs=secs, n8q=g, q=g + 4, n8r=g + 4 + n8q, r=g + 8 + n8q, num_vars=counts, num_public=counts + 4,
                domain_size=counts + 8, counts_end=counts + 12, prover_type=secs[1][0], ncoef=secs[4][0],
                first_section_size=16, nsections=8)


def with_coefficients(data, coefs):
    zk = CF.parse_zkey(data)
    return CF.write_zkey(zk["curve"], zk["num_vars"], zk["num_public"], zk["domain_size"], zk["vk"], zk["ic"], coefs,
                         zk["a1"], zk["b1"], zk["b2"], zk["c1"], zk["h1"])


def edge_words(r):
    """Coefficient words at the edges of the oracle's formula (word * R^-2 mod
    r, defined for every 256-bit word): zero, the value one (R^2 mod r, which
    the reference special-cases), and the words around r and at 2^256 - 1."""
    return [0, (1 << 512) % r, r - 1, r, r + 1, (1 << 256) - 1]


# ---- comparing a dump with the oracle ------------------------------------

def assert_zkey_dump(fields, data, name=""):
    zk = CF.parse_zkey(data)
    r = R_OF[zk["curve"]]
    assert fields["curve"] == zk["curve"], name
    assert fields["counts"].split() == [str(zk[k]) for k in ("num_vars", "num_public", "domain_size")], name
    for k, v in zk["vk"].items():
        assert fields[k] == v.hex(), (name, k)
    for k in ("ic", "a1", "b1", "b2", "c1", "h1"):
        assert fields[k] == b"".join(zk[k]).hex(), (name, k)
    got = [(int(m), int(c), int(s), int.from_bytes(bytes.fromhex(v), "little")) for m, c, s, v in fields["coef"]]
    want = [(m, c, s, CF.coefficient_value(w, r)) for m, c, s, w in zk["coefficients"]]
    assert got == want, name


def assert_wtns_dump(fields, values, r, name=""):
    """values: the integers in the file; the readers reduce them mod r."""
    assert int(fields["count"]) == len(values), name
    raw = bytes.fromhex(fields.get("values", ""))
    got = [int.from_bytes(raw[i * 32:(i + 1) * 32], "little") for i in range(len(values))]
    assert got == [v % r for v in values], name


# ---- valid files ----------------------------------------------------------

def test_valid_zkeys_match_the_oracle(exe, key3, tmp_path):
    z3, _ = key3
    r = P.BN254_FR
    zk3 = CF.parse_zkey(z3)
    n, m = zk3["domain_size"], zk3["num_vars"]
    words = [(i % 2, i % n, (i * 5) % m, w.to_bytes(32, "little")) for i, w in enumerate(edge_words(r))]
    secs = split_sections(z3)
    other_coefs = struct.pack("<I", 1) + struct.pack("<III", 0, 0, 0) + b"\x07" * 32
    blobs = {
        "multiplier_3.zkey": open(os.path.join(GOLDEN, "multiplier_3.zkey"), "rb").read(),
        "adder.zkey": open(os.path.join(GOLDEN, "adder.zkey"), "rb").read(),
        "synth3.zkey": z3,
        "edge_words.zkey": with_coefficients(z3, words),
        # matrix 2: the reference and the oracle treat every non-zero matrix as B
        "matrix2.zkey": with_coefficients(z3, zk3["coefficients"] + [(2, n - 1, m - 1, (12345).to_bytes(32, "little"))]),
        # a repeated section type keeps the first (sections.h MoveTo): a second 4 and a second 2 change nothing
        "duplicate.zkey": join_sections(b"zkey", 1, secs + [(4, other_coefs), (2, b"\x00" * 8)]),
    }
    assert CF.parse_zkey(blobs["duplicate.zkey"]) == zk3
    got = read_files(exe, "zkey", "bn254", blobs, tmp_path)
    for name, data in blobs.items():
        verdict, fields = got[name]
        assert verdict == "parsed", (name, verdict)
        assert_zkey_dump(fields, data, name)
    assert [c[0] for c in got["matrix2.zkey"][1]["coef"]].count("2") == 1

    zb, _ = synth_zkey("bls12_381", log_n=3, seed=32)
    rb = P.BLS12_381_FR
    bls_words = [(i % 2, i % 8, i % 6, w.to_bytes(32, "little")) for i, w in enumerate(edge_words(rb))]
    blobs = {"synth3_bls.zkey": zb, "edge_words_bls.zkey": with_coefficients(zb, bls_words)}
    got = read_files(exe, "zkey", "bls12_381", blobs, tmp_path)
    for name, data in blobs.items():
        verdict, fields = got[name]
        assert verdict == "parsed", (name, verdict)
        assert_zkey_dump(fields, data, name)


def test_valid_wtns_match_the_oracle(exe, key3, tmp_path):
    _, w3 = key3
    r = P.BN254_FR
    gold = open(os.path.join(GOLDEN, "multiplier_3.wtns"), "rb").read()
    # values >= r (write_wtns reduces, so they are patched in): today's readers reduce them mod r
    big = [1, r + 5, r, (1 << 256) - 1, r - 1, 0]
    over = CF.write_wtns([0] * len(big), r)
    body = CF._sections(over, 8)[2][0]
    over = patch(over, body, b"".join(v.to_bytes(32, "little") for v in big))
    blobs = {"multiplier_3.wtns": gold, "synth3.wtns": w3, "over_r.wtns": over}
    got = read_files(exe, "wtns", "bn254", blobs, tmp_path)
    for name in blobs:
        assert got[name][0] == "parsed", (name, got[name][0])
    assert_wtns_dump(got["multiplier_3.wtns"][1], CF.parse_wtns(gold, r), r)
    assert_wtns_dump(got["synth3.wtns"][1], CF.parse_wtns(w3, r), r)
    assert_wtns_dump(got["over_r.wtns"][1], big, r)
    rb = P.BLS12_381_FR
    wb = CF.write_wtns([1, rb - 1, 0, 77], rb)
    got = read_files(exe, "wtns", "bls12_381", {"bls.wtns": wb}, tmp_path)
    assert got["bls.wtns"][0] == "parsed"
    assert_wtns_dump(got["bls.wtns"][1], [1, rb - 1, 0, 77], rb)


# ---- refusals ---------------------------------------------------------------

def refused(verdict):
    return verdict.startswith("refused: circom:")


def test_zkey_refusals(exe, key3, tmp_path):
    z, _ = key3
    o = zkey_offsets(z)
    zk = CF.parse_zkey(z)
    n, m, npub = zk["domain_size"], zk["num_vars"], zk["num_public"]
    secs = split_sections(z)
    q, r = P.BN254_FQ, P.BN254_FR
    word = (3).to_bytes(32, "little")
    blobs = {
        "num_public_eq_num_vars": patch(z, o["num_public"], u32(m)),
        "domain_0": patch(z, o["domain_size"], u32(0)),
        "domain_3": patch(z, o["domain_size"], u32(3)),
        "magic": patch(z, 0, b"zkez"),
        "version": patch(z, 4, u32(2)),
        "prover_type_2": patch(z, o["prover_type"], u32(2)),
        "section_size_huge": patch(z, o["first_section_size"], struct.pack("<Q", 0xFFFFFFFFFFFFFFF0)),
        "section_count_huge": patch(z, o["nsections"], u32(0xFFFFFFFF)),
        "q_plus_1": patch(z, o["q"], (q + 1).to_bytes(32, "little")),
        "q_minus_1": patch(z, o["q"], (q - 1).to_bytes(32, "little")),
        "r_plus_1": patch(z, o["r"], (r + 1).to_bytes(32, "little")),
        "r_minus_1": patch(z, o["r"], (r - 1).to_bytes(32, "little")),
        "n8q_48": patch(z, o["n8q"], u32(48)),
        "bls_key": synth_zkey("bls12_381", log_n=3, seed=32)[0],
        "constraint_eq_domain": with_coefficients(z, zk["coefficients"] + [(0, n, 0, word)]),
        "signal_eq_num_vars": with_coefficients(z, zk["coefficients"] + [(1, 0, m, word)]),
    }
    for typ in range(1, 10):
        blobs[f"missing_section_{typ}"] = join_sections(b"zkey", 1, [s for s in secs if s[0] != typ])
    elem = {3: 64, 5: 64, 6: 64, 7: 128, 8: 64, 9: 64}
    assert npub + 1 > 0 and m - npub - 1 > 0
    for typ, size in elem.items():
        blobs[f"section_{typ}_one_short"] = join_sections(
            b"zkey", 1, [(t, b[:-size] if t == typ else b) for t, b in secs])
    got = read_files(exe, "zkey", "bn254", blobs, tmp_path)
    for name in blobs:
        assert refused(got[name][0]), (name, got[name][0])
    # (and each says what is wrong, not just that something is)
    assert "fewer variables" in got["num_public_eq_num_vars"][0]
    assert "power of two" in got["domain_0"][0] and "power of two" in got["domain_3"][0]
    assert "base field" in got["bls_key"][0] and "base field" in got["n8q_48"][0]
    assert "constraint" in got["constraint_eq_domain"][0] and "signal" in got["signal_eq_num_vars"][0]
    assert "missing section 7" in got["missing_section_7"][0]


def test_wtns_refusals(exe, key3, tmp_path):
    _, w = key3
    secs = split_sections(w)
    mod_at = CF._sections(w, 8)[1][0] + 4
    assert w[mod_at:mod_at + 32] == P.BN254_FR.to_bytes(32, "little")
    blobs = {
        "magic": patch(w, 0, b"wtnz"),
        "version": patch(w, 4, u32(1)),
        "wrong_modulus": CF.write_wtns([1, 2, 3], P.BLS12_381_FR),
        "modulus_plus_1": patch(w, mod_at, (P.BN254_FR + 1).to_bytes(32, "little")),
        "data_one_byte_short": join_sections(b"wtns", 2, [(t, b[:-1] if t == 2 else b) for t, b in secs]),
        "missing_section_2": join_sections(b"wtns", 2, [s for s in secs if s[0] != 2]),
    }
    got = read_files(exe, "wtns", "bn254", blobs, tmp_path)
    for name in blobs:
        assert refused(got[name][0]), (name, got[name][0])


def test_huge_counts_are_refused_without_allocating(exe, key3, tmp_path):
    """Each patched count in a child of its own: refused by the readers, and
    the child's peak RSS within 64 MiB of the valid parse's -- both as wait4
    reports it (which never falls below this process's own size at the fork)
    and as the child reads it from its own VmHWM."""
    z, w = key3
    o = zkey_offsets(z)
    wtns_count = CF._sections(w, 8)[1][0] + 4 + 32
    cases = [
        ("zkey", "num_vars_2_26", patch(z, o["num_vars"], u32(1 << 26))),
        ("zkey", "ncoef_2_27", patch(z, o["ncoef"], u32(1 << 27))),
        ("zkey", "domain_2_31", patch(z, o["domain_size"], u32(1 << 31))),
        ("zkey", "ncoef_ffffffff", patch(z, o["ncoef"], u32(0xFFFFFFFF))),
        ("zkey", "num_public_ffffffff", patch(z, o["num_public"], u32(0xFFFFFFFF))),
        ("wtns", "wtns_count_2_28", patch(w, wtns_count, u32(1 << 28))),
    ]
    base = {}
    for kind, data in (("zkey", z), ("wtns", w)):
        p = tmp_path / f"valid.{kind}"
        p.write_bytes(data)
        code, out, err, rss = run(exe, [kind, "bn254", p], tmp_path)
        assert code == 0 and records(out)[0][1] == "parsed", out[-500:] + err[-2000:]
        base[kind] = (rss, own_peak(out))
    for kind, name, data in cases:
        p = tmp_path / name
        p.write_bytes(data)
        code, out, err, rss = run(exe, [kind, "bn254", p], tmp_path)
        recs = records(out)
        assert code == 0 and len(recs) == 1 and refused(recs[0][1]), (name, code, out[-500:], err[-2000:])
        print(f"{name}: peak RSS {rss} / {own_peak(out)} KiB (valid {kind}: {base[kind]} KiB)")
        assert rss <= base[kind][0] + RSS_CAP_KIB, (name, rss, base[kind])
        assert own_peak(out) <= base[kind][1] + RSS_CAP_KIB, (name, own_peak(out), base[kind])


# ---- sweeps, each in one process -------------------------------------------

def test_every_proper_prefix_is_refused(exe, key3, tmp_path):
    z, w = key3
    for kind, data in (("zkey", z), ("wtns", w)):
        p = tmp_path / f"whole.{kind}"
        p.write_bytes(data)
        code, out, err, _ = run(exe, ["prefixes", kind, "bn254", p], tmp_path)
        assert code == 0, out[-2000:] + err[-4000:]
        assert out.splitlines()[-1] == f"prefixes {len(data)} refused {len(data)}", out[-2000:]


def test_header_byte_mutations_parse_or_are_refused(exe, key3, tmp_path):
    """Every byte up to the end of section 2's counts and every byte of the
    coefficient count, set to 0x00, 0xFF and its value -1 / +1: the readers
    parse or refuse, never anything else (any sanitizer report ends the
    process before the summary line)."""
    z, _ = key3
    o = zkey_offsets(z)
    p = tmp_path / "whole.zkey"
    p.write_bytes(z)
    code, out, err, _ = run(exe, ["mutate", "bn254", p, 0, o["counts_end"], o["ncoef"], o["ncoef"] + 4], tmp_path)
    assert code == 0, out[-2000:] + err[-4000:]
    words = out.splitlines()[-1].split()
    assert words[0::2] == ["mutations", "parsed", "refused", "errors"], out[-2000:]
    total, parsed, refused_n, errors = (int(x) for x in words[1::2])
    nbytes = o["counts_end"] + 4
    assert errors == 0 and parsed + refused_n == total and 3 * nbytes <= total <= 4 * nbytes
    assert refused_n > parsed  # (most header bytes matter)


def test_makefile_builds_the_check():
    r = subprocess.run(["make", "-s", "-n", "-C", CSRC, "../bin/circom_io_check"], capture_output=True, text=True)
    assert r.returncode == 0 and "circom_io_check.cc" in r.stdout and "--offload-host-only" in r.stdout, r.stderr
    r = subprocess.run(["make", "-s", "-n", "-C", CSRC, "all"], capture_output=True, text=True)
    assert "circom_io_check" not in r.stdout
