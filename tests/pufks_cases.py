"""Shapes, inputs, references and bounds of the public functional keyswitch (`public_functional_keyswitch`, sunscreen_tfhe
ops/keyswitch/public_functional_keyswitch.rs:74-148, map "message j to coefficient j"), shared by
tests/test_public_functional_keyswitch_reference.py (CPU) and tests/test_gpu_public_functional_keyswitch.py.  No GPU here.

p LWEs (a_j, b_j) of dimension n -> one GLWE: poly_i = sum_j a_j[i] X^j; acc_fft += <Decomp(poly_i), fft(K[i])> for i ascending
(`decomposed_polynomial_glev_mad`, ops/fft_ops.rs:67-98); out = -(ifft(acc_fft)); out.body[j] += b_j.  The loop over i is
`glwe_ggsw_mad` over consecutive groups of k+1 key rows into one spectrum, which is how `pufks_oracle` states it: rows padded with
zero polynomials and zero key rows to a multiple of k+1 (a zero digit polynomial adds exact zeros)."""
import functools

import numpy as np

import oracle as O
from tests import poly_ref as R
from tests.polyref_cases import NOISE, Case, sigma_model

# tier A, class uniform: (N, k, n, count, log, p, seed)
TIER_A = [(128, 2, 7, 3, 4, 5, 1), (128, 2, 16, 3, 4, 128, 2), (2048, 1, 5, 8, 4, 3, 3), (2048, 1, 64, 4, 4, 2048, 4),
          (2048, 1, 64, 8, 4, 65, 5)]
# meaning, honest key: (N, k, n, count, log)
MEANING = [(128, 2, 16, 3, 4), (2048, 1, 32, 4, 4)]


def input_polys(lwes, N: int) -> np.ndarray:
    """(p, n + 1) LWE rows -> the n input polynomials (n, N): coefficient j of poly_i is word i of row j, zeros from p on"""
    lwes = np.asarray(lwes, dtype=np.uint64)
    p, n = lwes.shape[0], lwes.shape[1] - 1
    assert 1 <= p <= N
    polys = np.zeros((n, N), dtype=np.uint64)
    polys[:, :p] = lwes[:, :n].T
    return polys


def pufks_oracle(lwes, key_fft_, N: int, k: int, radix_log: int, count: int) -> np.ndarray:
    """the operation in the oracle's arithmetic, bit for bit: (k+1, N) words.  key_fft_: [n][count][k+1][N/2] complex, flat or not"""
    lwes = np.asarray(lwes, dtype=np.uint64)
    p, n = lwes.shape[0], lwes.shape[1] - 1
    h = N // 2
    groups = -(-n // (k + 1))
    polys = np.zeros((groups * (k + 1), N), dtype=np.uint64)
    polys[:n] = input_polys(lwes, N)
    keyf = np.zeros((groups, (k + 1) * count * (k + 1) * h), dtype=np.complex128)
    keyf.reshape(-1)[:n * count * (k + 1) * h] = np.asarray(key_fft_, dtype=np.complex128).reshape(-1)
    acc = np.zeros((k + 1) * h, dtype=np.complex128)
    for g in range(groups):
        acc = O.glwe_ggsw_mad(acc, polys[g * (k + 1):(g + 1) * (k + 1)].reshape(-1), keyf[g], N, k, radix_log, count)
    out = np.stack([np.uint64(0) - O.poly_ifft(acc[q * h:(q + 1) * h]) for q in range(k + 1)])
    out[k, :p] += lwes[:, n]
    return out


def pufks_exact(lwes, key, radix_log: int, count: int, be=R.EXACT) -> np.ndarray:
    """the same sum over the ring (be = R.EXACT) or through numpy's FFT (R.NUMPY); key: (n, count, k+1, N) time-domain words"""
    lwes, key = np.asarray(lwes, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    p, n = lwes.shape[0], lwes.shape[1] - 1
    assert key.shape[:2] == (n, count)
    k, N = key.shape[2] - 1, key.shape[3]
    D = R._glev_digits(input_polys(lwes, N), radix_log, count).reshape(1, n * count, N)
    out = np.uint64(0) - be.sum_products(D, key.reshape(n * count, k + 1, N))[0]
    out[k, :p] += lwes[:, n]
    return out


def uniform_inputs(seed, N, k, n, log, count, p):
    """(key (n, count, k+1, N), lwes (p, n+1)), uniform words"""
    rng = np.random.default_rng([seed, N, k, n, log, count, p])
    key = rng.integers(0, 1 << 64, (n, count, k + 1, N), dtype=np.uint64)
    return key, rng.integers(0, 1 << 64, (p, n + 1), dtype=np.uint64)


def tier_a_name(shape) -> str:
    N, k, n, count, log, p, _ = shape
    return f"pufks-N{N}k{k}-n{n}-{count}x{log}-p{p}"


@functools.lru_cache(maxsize=None)
def tier_a_case(shape):
    """(Case, lwes, exact words, numpy-pipeline words) of a TIER_A shape, computed once in a process and left unchanged"""
    N, k, n, count, log, p, seed = shape
    key, lwes = uniform_inputs(seed, N, k, n, log, count, p)
    c = Case(tier_a_name(shape), "uniform", None, key, sigma=sigma_model(log, n * count, N))
    return c, lwes, pufks_exact(lwes, key, log, count), pufks_exact(lwes, key, log, count, R.NUMPY)


def honest_key(rng, lwe_sk, glwe_sk, N: int, radix_log: int, count: int) -> np.ndarray:
    """row (i, lvl) = glwe_encrypt of the constant polynomial s_i * 2^(64 - log (lvl + 1)): (n, count, k+1, N)"""
    lwe_sk = np.asarray(lwe_sk, dtype=np.uint64)
    n = lwe_sk.size
    msgs = np.zeros((n, count, N), dtype=np.uint64)
    for lvl in range(count):
        msgs[:, lvl, 0] = lwe_sk << np.uint64(64 - radix_log * (lvl + 1))
    k = np.asarray(glwe_sk).size // N
    return R.glwe_encrypt(rng, glwe_sk, msgs.reshape(n * count, N), NOISE).reshape(n, count, k + 1, N)


def lwe_phases(lwes, lwe_sk) -> np.ndarray:
    """b_j - <a_j, s> of every row"""
    lwes = np.asarray(lwes, dtype=np.uint64)
    return lwes[:, -1] - (lwes[:, :-1] * np.asarray(lwe_sk, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def meaning_bounds(n: int, count: int, log: int, p: int):
    """(bound on coefficients j < p, bound on coefficients >= p), in units of the torus.  Derived, not measured: the
    decomposition drops at most half a unit of the last digit from each of the n mask words, n * 2^-(count log + 1); every one of
    the n * count key rows carries noise |e| <= NOISE in each coefficient, multiplied by a digit polynomial of at most p
    non-zero coefficients of magnitude <= 2^(log - 1): n * count * p * 2^(log - 1) * NOISE / 2^64."""
    noise = n * count * p * 2.0 ** (log - 1) * NOISE / 2.0 ** 64
    return n * 2.0 ** -(count * log + 1) + noise, noise


def check_meaning(out, lwes, lwe_sk, glwe_sk, count: int, log: int, who: str):
    """the phase of `out` (k+1, N) holds the phase of LWE j at coefficient j < p and nothing beyond"""
    lwes = np.asarray(lwes, dtype=np.uint64)
    p, n = lwes.shape[0], lwes.shape[1] - 1
    ph = R.glwe_phase(out, glwe_sk)
    lo, hi = meaning_bounds(n, count, log, p)
    d = R.torus_distance(ph[:p], lwe_phases(lwes, lwe_sk))
    rest = R.torus_distance(ph[p:], np.zeros(ph.size - p, dtype=np.uint64)) if p < ph.size else np.zeros(1)
    print(f"pufks meaning n={n} {count}x{log} p={p} {who:6s} distance max 2^{np.log2(max(d.max(), 2.0 ** -80)):.2f} (bound "
          f"2^{np.log2(lo):.2f}); beyond p max 2^{np.log2(max(rest.max(), 2.0 ** -80)):.2f} (bound 2^{np.log2(hi):.2f})")
    assert d.max() <= lo, (who, n, p, float(d.max()), lo)
    assert rest.max() <= hi, (who, n, p, float(rest.max()), hi)


@functools.lru_cache(maxsize=None)
def meaning_keys(shape):
    """(lwe_sk, glwe_sk, honest key) of a MEANING shape, built once in a process"""
    N, k, n, count, log = shape
    rng = np.random.default_rng([0xB5, N, k, n, log, count])
    lwe_sk, glwe_sk = R.binary_key(rng, n), R.binary_key(rng, k * N)
    return lwe_sk, glwe_sk, honest_key(rng, lwe_sk, glwe_sk, N, log, count)


def meaning_lwes(shape, p: int) -> np.ndarray:
    N, k, n, count, log = shape
    return np.random.default_rng([0xB6, N, k, n, log, count, p]).integers(0, 1 << 64, (p, n + 1), dtype=np.uint64)
