"""The reference the BabyBear GPU tests compare against: numpy uint64
arithmetic plus Python integers, a few lines per function.  It imports neither
the library nor the oracle.

Everything works directly on the stored Montgomery words with canonical
twiddles: the transform is linear over the field, so x -> x R commutes with it
and only the generator and the shift a caller hands to the library need
converting (mont()).
"""
import numpy as np

P = 2**31 - 2**27 + 1          # 2013265921 = 0x78000001
R = 2**32                      # Montgomery radix
GENERATOR = 31
TWO_ADICITY = 27
_P = np.uint64(P)


def mont(x: int) -> int:
    return (x % P) * R % P


def from_mont(x: int) -> int:
    return (x % P) * pow(R, -1, P) % P


def root_of_unity(n: int) -> int:
    """w_n = 31^((p-1)/n), canonical."""
    assert n >= 1 and n & (n - 1) == 0 and n <= 1 << TWO_ADICITY
    return pow(GENERATOR, (P - 1) // n, P)


def _powers(b: int, n: int) -> np.ndarray:
    """[b^0 .. b^(n-1)] mod p as uint64, by doubling."""
    out = np.ones(n, dtype=np.uint64)
    k, bk = 1, b % P               # out[:k] is done, bk = b^k
    while k < n:
        m = min(k, n - k)
        out[k:k + m] = out[:m] * np.uint64(bk) % _P
        k, bk = 2 * k, bk * bk % P
    return out


def _as_u64(words) -> np.ndarray:
    a = np.asarray(words, dtype=np.uint64)
    assert a.ndim in (1, 2) and (a < _P).all()
    return a


def _scale_rows(x: np.ndarray, factors: np.ndarray) -> np.ndarray:
    f = factors if x.ndim == 1 else factors[:, None]
    return x * f % _P          # both < 2^31: the product fits uint64


def dft(words, w: int) -> np.ndarray:
    """X[i] = sum_j x[j] w^(i j) along axis 0 (length n a power of two, w of
    order n), vectorised over an optional trailing column axis.  Radix-2
    decimation in time: bit-reversed rows, then log n butterfly stages."""
    x = _as_u64(words)
    n = x.shape[0]
    assert n >= 1 and n & (n - 1) == 0
    bits = n.bit_length() - 1
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        rev |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    y = x[rev].reshape(n, -1)
    h = 1
    while h < n:
        tw = _powers(pow(w, n // (2 * h), P), h)[None, :, None]
        v = y.reshape(n // (2 * h), 2, h, -1)
        a, b = v[:, 0], v[:, 1] * tw % _P
        y = np.stack([(a + b) % _P, (a + _P - b) % _P], axis=1).reshape(n, -1)
        h *= 2
    return y.reshape(x.shape)


def fft(words, coset: int = 1, w: int = None) -> np.ndarray:
    """Evaluations at coset * w_n^i, natural order; w: a root of order n other
    than w_n."""
    x = _as_u64(words)
    n = x.shape[0]
    if coset % P != 1:
        x = _scale_rows(x, _powers(coset % P, n))
    return dft(x, root_of_unity(n) if w is None else w)


def ifft(words, coset: int = 1, w: int = None) -> np.ndarray:
    """Coefficients from the evaluations at coset * w_n^i."""
    x = _as_u64(words)
    n = x.shape[0]
    w = root_of_unity(n) if w is None else w
    y = _scale_rows(dft(x, pow(w, -1, P)), np.full(n, pow(n, -1, P), dtype=np.uint64))
    if coset % P != 1:
        y = _scale_rows(y, _powers(pow(coset, -1, P), n))
    return y


def coset_lde(mat, added_bits: int, shift: int) -> np.ndarray:
    """CosetLDEBatch from its definition, per column: interpolate on the plain
    domain of size rows, scale coefficient j by shift^j, zero-pad to
    rows << added_bits, evaluate on the plain domain of that size."""
    x = _as_u64(mat)
    rows = x.shape[0]
    coeffs = _scale_rows(ifft(x), _powers(shift % P, rows))
    padded = np.zeros((rows << added_bits,) + x.shape[1:], dtype=np.uint64)
    padded[:rows] = coeffs
    return fft(padded)


def to_bytes(words) -> bytes:
    return np.asarray(words, dtype=np.uint64).astype("<u4").tobytes()


def from_bytes(data: bytes, cols: int = None) -> np.ndarray:
    a = np.frombuffer(data, dtype="<u4").astype(np.uint64)
    return a if cols is None else a.reshape(-1, cols)
