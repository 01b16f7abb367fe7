"""The reference the Poseidon2 / FieldMerkleTree GPU tests compare against:
numpy uint64 arithmetic vectorised over rows plus Python integers.  It imports
neither the library nor the oracle.

Everything here works on canonical field elements of BabyBear
(p = 2^31 - 2^27 + 1).  The library stores Montgomery words (R = 2^32);
mont_words() / from_mont_words() convert whole arrays at the boundary.

Configuration (the one the reference uses everywhere): Poseidon2 of width 16,
alpha = 7, 8 full and 13 partial rounds, PaddingFreeSponge<16, 8, 8> leaf
hashes, TruncatedPermutation<16, 8, 2> compression, FieldMerkleTree<F, 8>.
"""
import numpy as np

P = 2**31 - 2**27 + 1
R = 2**32
WIDTH = 16
RATE = 8
DIGEST = 8
ALPHA = 7
FULL_ROUNDS = 8
PARTIAL_ROUNDS = 13
SHIFTS = tuple(range(14)) + (15,)          # lanes 1..15 of the internal layer
M4 = {
    "horizen": ((5, 7, 1, 3), (4, 6, 1, 1), (1, 3, 5, 7), (1, 1, 4, 6)),
    "plonky3": ((2, 3, 1, 1), (1, 2, 3, 1), (1, 1, 2, 3), (3, 1, 1, 2)),
}
_P = np.uint64(P)
_RINV = pow(R, -1, P)


def mont_words(x) -> np.ndarray:
    """canonical -> stored Montgomery words"""
    return np.asarray(x, dtype=np.uint64) * np.uint64(R % P) % _P


def from_mont_words(w) -> np.ndarray:
    """stored Montgomery words -> canonical"""
    return np.asarray(w, dtype=np.uint64) * np.uint64(_RINV) % _P


# ---------------------------------------------------------------- constants

def grain_lfsr_elements(count: int):
    """`count` field elements from the Grain LFSR of the Poseidon papers with
    the parameters of this configuration."""
    bits = []

    def put(value, width):
        bits.extend((value >> (width - 1 - i)) & 1 for i in range(width))

    put(1, 2)                      # prime field
    put(0, 4)                      # s-box x^alpha
    put(31, 12)                    # modulus bits
    put(WIDTH, 12)
    put(FULL_ROUNDS, 10)
    put(PARTIAL_ROUNDS, 10)
    put((1 << 30) - 1, 30)
    assert len(bits) == 80
    state = bits

    def update():
        b = state[62] ^ state[51] ^ state[38] ^ state[23] ^ state[13] ^ state[0]
        state.pop(0)
        state.append(b)
        return b

    for _ in range(160):
        update()

    def kept_bit():
        while True:
            first, second = update(), update()
            if first:
                return second

    out = []
    while len(out) < count:
        v = 0
        for _ in range(31):
            v = (v << 1) | kept_bit()
        if v < P:
            out.append(v)
    return out


_ARK = None


def round_constants():
    """ark[r]: 16 canonical constants for the full rounds (0-3, 17-20), one
    (lane 0) for the partial rounds (4-16)."""
    global _ARK
    if _ARK is None:
        half = FULL_ROUNDS // 2
        sizes = [WIDTH] * half + [1] * PARTIAL_ROUNDS + [WIDTH] * half
        flat = grain_lfsr_elements(sum(sizes))
        _ARK, at = [], 0
        for s in sizes:
            _ARK.append(flat[at:at + s])
            at += s
    return _ARK


# ---------------------------------------------------------------- layers

def external_matrix(external: str) -> np.ndarray:
    """The 16 x 16 matrix of the external layer: every 4 x 4 block is M4, the
    diagonal blocks twice."""
    m4 = np.array(M4[external], dtype=np.uint64)
    m = np.tile(m4, (4, 4))
    for b in range(4):
        m[4 * b:4 * b + 4, 4 * b:4 * b + 4] += m4
    return m


def internal_matrix() -> np.ndarray:
    """(J + diag(-2, 2^shifts)) 2^-32 as canonical entries"""
    m = np.ones((WIDTH, WIDTH), dtype=object)
    m[0, 0] += P - 2
    for i in range(1, WIDTH):
        m[i, i] += 1 << SHIFTS[i - 1]
    return np.array([[int(v) * _RINV % P for v in row] for row in m], dtype=np.uint64)


def external_layer(s: np.ndarray, external: str) -> np.ndarray:
    """Step 1: M4 on each block of 4 lanes.  Step 2: lane i += the sum of the
    lanes congruent to i mod 4."""
    m4 = M4[external]
    n = s.shape[0]
    b = s.reshape(n, 4, 4)
    t = np.zeros_like(b)
    for r in range(4):
        acc = np.zeros((n, 4), dtype=np.uint64)
        for c in range(4):
            acc += np.uint64(m4[r][c]) * b[:, :, c]
        t[:, :, r] = acc % _P
    sums = t.sum(axis=1) % _P                     # (n, 4): per residue mod 4
    return ((t + sums[:, None, :]) % _P).reshape(n, WIDTH)


def internal_layer(s: np.ndarray) -> np.ndarray:
    total = s.sum(axis=1)
    out = np.empty_like(s)
    out[:, 0] = (total + np.uint64(2) * (_P - s[:, 0])) % _P
    for i in range(1, WIDTH):
        out[:, i] = (total + (s[:, i] << np.uint64(SHIFTS[i - 1]))) % _P
    return out * np.uint64(_RINV) % _P


def _sbox(x: np.ndarray) -> np.ndarray:
    x2 = x * x % _P
    x3 = x2 * x % _P
    x4 = x2 * x2 % _P
    return x3 * x4 % _P


def permute(states, external: str = "horizen") -> np.ndarray:
    """Poseidon2 on an (n, 16) array of canonical states."""
    s = np.array(states, dtype=np.uint64).reshape(-1, WIDTH)
    assert (s < _P).all()
    ark = round_constants()
    half = FULL_ROUNDS // 2
    s = external_layer(s, external)
    for r in range(half + PARTIAL_ROUNDS + half):
        if half <= r < half + PARTIAL_ROUNDS:
            s[:, 0] = _sbox((s[:, 0] + np.uint64(ark[r][0])) % _P)
            s = internal_layer(s)
        else:
            s = _sbox((s + np.array(ark[r], dtype=np.uint64)[None, :]) % _P)
            s = external_layer(s, external)
    return s


# ---------------------------------------------------------------- hash, compress

def hash_rows(rows, external: str = "horizen") -> np.ndarray:
    """PaddingFreeSponge<16, 8, 8> of every row of an (n, cols) array: chunks
    of 8 overwrite the rate lanes, a short last chunk leaves the others."""
    x = np.array(rows, dtype=np.uint64)
    assert x.ndim == 2 and (x < _P).all()
    n, cols = x.shape
    s = np.zeros((n, WIDTH), dtype=np.uint64)
    for at in range(0, cols, RATE):
        k = min(RATE, cols - at)
        s[:, :k] = x[:, at:at + k]
        s = permute(s, external)
    return s[:, :DIGEST].copy()


def compress(left, right, external: str = "horizen") -> np.ndarray:
    """TruncatedPermutation<16, 8, 2> on (n, 8) digests."""
    s = np.concatenate([np.asarray(left, dtype=np.uint64), np.asarray(right, dtype=np.uint64)], axis=1)
    return permute(s, external)[:, :DIGEST].copy()


# ---------------------------------------------------------------- tree

def bit_ceil(n: int) -> int:
    return 1 << (n - 1).bit_length() if n > 1 else 1


def ceil_log2(n: int) -> int:
    return (n - 1).bit_length() if n > 1 else 0


def bit_reverse_rows(mat) -> np.ndarray:
    x = np.asarray(mat)
    n = x.shape[0]
    assert n & (n - 1) == 0
    bits = n.bit_length() - 1
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        rev |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return x[rev]


def heights_ok(heights) -> bool:
    """matrix heights that round up to the same power of two must be equal"""
    seen = {}
    for h in heights:
        if h < 1 or seen.setdefault(bit_ceil(h), h) != h:
            return False
    return True


def build(mats, external: str = "horizen", bit_reversed: bool = False):
    """FieldMerkleTree::Build: the digest layers, layer 0 first, each an
    (size, 8) canonical array."""
    mats = [np.asarray(m, dtype=np.uint64) for m in mats]
    assert mats and all(m.ndim == 2 and m.shape[1] >= 1 for m in mats)
    assert heights_ok([m.shape[0] for m in mats])
    if bit_reversed:
        mats = [bit_reverse_rows(m) for m in mats]
    order = sorted(range(len(mats)), key=lambda i: -mats[i].shape[0])      # stable
    rest = [mats[i] for i in order]

    def take(size):
        group = []
        while rest and bit_ceil(rest[0].shape[0]) == size:
            group.append(rest.pop(0))
        return group

    size = bit_ceil(rest[0].shape[0])
    group = take(size)
    rows = group[0].shape[0]
    layer = np.zeros((size, DIGEST), dtype=np.uint64)
    layer[:rows] = hash_rows(np.concatenate(group, axis=1), external)
    layers = [layer]
    while size > 1:
        size //= 2
        nxt = compress(layer[0::2], layer[1::2], external)
        group = take(size)
        if group:
            rows = group[0].shape[0]
            inject = np.zeros((size, DIGEST), dtype=np.uint64)
            inject[:rows] = hash_rows(np.concatenate(group, axis=1), external)
            nxt = compress(nxt, inject, external)
        layer = nxt
        layers.append(layer)
    assert not rest
    return layers


def open_at(mats, layers, index: int, bit_reversed: bool = False):
    """DoCreateOpeningProof: (opened row of every matrix in the caller's order,
    siblings).  A row past a matrix's height (padded part) opens as zeros."""
    log_max = len(layers) - 1
    assert 0 <= index < (1 << log_max)
    opened = []
    for m in mats:
        m = np.asarray(m, dtype=np.uint64)
        lg = ceil_log2(m.shape[0])
        r = index >> (log_max - lg)
        if bit_reversed:
            r = int(format(r, "b").zfill(lg)[::-1], 2) if lg else 0
        opened.append(m[r].copy() if r < m.shape[0] else np.zeros(m.shape[1], dtype=np.uint64))
    siblings = [layers[k][(index >> k) ^ 1].copy() for k in range(log_max)]
    return opened, siblings


def verify(root, dims, index: int, opened, siblings, external: str = "horizen") -> bool:
    """DoVerifyOpeningProof: dims are (rows, cols) per matrix in the caller's
    order."""
    order = sorted(range(len(dims)), key=lambda i: -dims[i][0])
    rest = list(order)

    def take(size):
        group = []
        while rest and bit_ceil(dims[rest[0]][0]) == size:
            group.append(rest.pop(0))
        return group

    def hash_group(group):
        row = np.concatenate([np.asarray(opened[i], dtype=np.uint64) for i in group])
        return hash_rows(row[None, :], external)

    size = bit_ceil(dims[rest[0]][0])
    cur = hash_group(take(size))
    for sib in siblings:
        sib = np.asarray(sib, dtype=np.uint64)[None, :]
        cur = compress(cur, sib, external) if index & 1 == 0 else compress(sib, cur, external)
        index >>= 1
        size >>= 1
        group = take(size)
        if group:
            cur = compress(cur, hash_group(group), external)
    return bool((cur[0] == np.asarray(root, dtype=np.uint64)).all())


def to_bytes(words) -> bytes:
    return np.asarray(words, dtype=np.uint64).astype("<u4").tobytes()


def from_bytes(data: bytes, cols: int = None) -> np.ndarray:
    a = np.frombuffer(data, dtype="<u4").astype(np.uint64)
    return a if cols is None else a.reshape(-1, cols)
