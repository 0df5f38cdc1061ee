"""An independent statement of the gadget decomposition and of the LWE keyswitch (test infrastructure).

Neither the oracle nor the library is called here: the digits are restated on Python integers from the reference's
definitions (sunscreen_tfhe/src/math/radix.rs:157-162 `round`, math/simd/scalar.rs:52-71 `vector_next_decomp`), and the
keyswitch (ops/keyswitch/lwe_keyswitch.rs:23-62) is one wrapping uint64 matrix product over those digits.  Both the oracle and
the HIP kernels are held to it at every radix the ABI accepts.
"""
import numpy as np

M64 = (1 << 64) - 1


def radix_round(x: int, radix_log: int, count: int) -> int:
    """x rounded to its top radix_log * count bits, as an integer of that many bits (plus a possible carry out)"""
    assert 1 <= radix_log and 1 <= count and radix_log * count < 64
    shift = 64 - radix_log * count
    x &= M64
    return (x >> shift) + ((x >> (shift - 1)) & 1)


def radix_digits(x: int, radix_log: int, count: int) -> list:
    """signed digits of x, least significant first, each in [-2^(logB-1), 2^(logB-1) - 1]"""
    st = radix_round(x, radix_log, count)
    mask = (1 << radix_log) - 1
    out = []
    for _ in range(count):
        d = st & mask
        st >>= radix_log
        carry = d >> (radix_log - 1)
        st += carry
        out.append(d - (carry << radix_log))
    return out


def recompose(digits, radix_log: int) -> int:
    """sum_j d_j 2^(64 - logB*count + logB*j) mod 2^64: the word the digits stand for"""
    shift = 64 - radix_log * len(digits)
    return sum(d << (shift + radix_log * j) for j, d in enumerate(digits)) & M64


def round_to_grid(x: int, radix_log: int, count: int) -> int:
    """x rounded to the nearest multiple of 2^(64 - logB*count), mod 2^64"""
    return (radix_round(x, radix_log, count) << (64 - radix_log * count)) & M64


def digits_array(x: np.ndarray, radix_log: int, count: int) -> np.ndarray:
    """radix_digits of every word of x (any shape) in wrapping uint64: shape x.shape + (count,), int64"""
    assert 1 <= radix_log and 1 <= count and radix_log * count < 64
    x = np.asarray(x, dtype=np.uint64)
    shift = np.uint64(64 - radix_log * count)
    st = (x >> shift) + ((x >> (shift - np.uint64(1))) & np.uint64(1))
    mask, L = np.uint64((1 << radix_log) - 1), np.uint64(radix_log)
    out = np.empty(x.shape + (count,), dtype=np.int64)
    for j in range(count):
        d = st & mask
        st = st >> L
        carry = d >> (L - np.uint64(1))
        st = st + carry
        out[..., j] = d.astype(np.int64) - (carry.astype(np.int64) << np.int64(radix_log))
    return out


def keyswitch_ref(ct, ksk, n_in: int, n_out: int, radix_log: int, count: int) -> np.ndarray:
    """(0, ..., 0, b) - sum_i sum_j d_ij * KSK[i][count - 1 - j]  mod 2^64, for one ciphertext (n_in + 1,) or a batch
    (B, n_in + 1); KSK laid out [n_in][count][n_out + 1] as the oracle and the library take it."""
    ct = np.asarray(ct, dtype=np.uint64)
    single = ct.ndim == 1
    ct = ct.reshape(-1, n_in + 1)
    w = n_out + 1
    key = np.asarray(ksk, dtype=np.uint64).reshape(n_in, count, w)[:, ::-1, :].reshape(n_in * count, w)
    d = digits_array(ct[:, :n_in], radix_log, count).reshape(ct.shape[0], n_in * count).view(np.uint64)
    out = np.zeros((ct.shape[0], w), dtype=np.uint64)
    out -= d @ key
    out[:, n_out] += ct[:, n_in]
    return out[0] if single else out


def lwe_phase(ct, sk) -> np.ndarray:
    """b - <a, s> mod 2^64 of one LWE ciphertext or of a batch"""
    ct, sk = np.asarray(ct, dtype=np.uint64), np.asarray(sk, dtype=np.uint64)
    n = sk.size
    return ct[..., n] - (ct[..., :n] * sk).sum(axis=-1, dtype=np.uint64)


def noiseless_keyswitch_phase(ct, sk_in, radix_log: int, count: int) -> np.ndarray:
    """what a keyswitch under a noiseless key must decrypt to: b - sum_i s_in[i] * round_{2^(64 - logB*count)}(a_i)"""
    ct, sk_in = np.asarray(ct, dtype=np.uint64), np.asarray(sk_in, dtype=np.uint64)
    n = sk_in.size
    a = ct[..., :n]
    shift = np.uint64(64 - radix_log * count)
    rounded = ((a >> shift) + ((a >> (shift - np.uint64(1))) & np.uint64(1))) << shift
    return ct[..., n] - (rounded * sk_in).sum(axis=-1, dtype=np.uint64)


def extreme_words(radix_log: int, count: int) -> list:
    """0, 2^63, 2^64 - 1 and the words recomposed from digit vectors at the ends of the digit range"""
    lo, hi = -(1 << (radix_log - 1)), (1 << (radix_log - 1)) - 1
    words = [0, 1 << 63, M64]
    for ds in ([lo] * count, [hi] * count, [lo if j % 2 else hi for j in range(count)],
               [hi if j % 2 else lo for j in range(count)]):
        words.append(recompose(ds, radix_log))
    return words
