"""Shapes, inputs, references and bounds of the private functional keyswitch (`private_functional_keyswitch`, sunscreen_tfhe
ops/keyswitch/private_functional_keyswitch.rs:107-142) and of the pieces of `circuit_bootstrap_via_pfks`
(ops/bootstrapping/circuit_bootstrapping.rs:162-252, :485-514), shared by tests/test_private_functional_keyswitch_reference.py
(CPU) and tests/test_gpu_private_functional_keyswitch.py.  No GPU and no oracle here: numpy and Python integers only.

p LWEs ct_z = (a_z, b_z) of dimension n and a key K[z][i][lvl] (GLWEs of (k+1) N words, i <= n):
    out = - sum_z sum_{i <= n} sum_j digit_j(ct_z[i]) * K[z][i][count-1-j]        (every word mod 2^64)
The body word is row i = n and is decomposed like the mask words; no body is added afterwards."""
import numpy as np

from tests import poly_ref as R
from tests.decomp_ref import M64, digits_array, extreme_words, radix_digits
from tests.polyref_cases import NOISE

# log x count, every class of the dispatcher: one limb (<= 8 bits), two (9..15), three (16..23), none (>= 24: VALU)
RADICES = [(4, 3), (8, 2), (9, 2), (11, 3), (16, 2), (17, 2), (23, 2), (24, 2), (31, 2), (63, 1), (7, 9)]
PLANTED = [0, M64, 1 << 63, 0x8080808080808080]


def pfks_ref(lwes, key, radix_log: int, count: int) -> np.ndarray:
    """one wrapping uint64 matrix product over decomp_ref.digits_array, in the shape of decomp_ref.keyswitch_ref.
    lwes (p, n+1) or (B, p, n+1); key (p, n+1, count, k+1, N); returns ((k+1) N,) or (B, (k+1) N)"""
    lwes, key = np.asarray(lwes, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    single = lwes.ndim == 2
    x = lwes.reshape((-1,) + lwes.shape[-2:])
    p, rows = x.shape[1], x.shape[2]
    assert key.shape[:3] == (p, rows, count), (key.shape, x.shape, count)
    w = key.shape[3] * key.shape[4]
    rev = key[:, :, ::-1].reshape(p * rows * count, w)                       # digit j meets level count - 1 - j
    d = digits_array(x, radix_log, count).reshape(x.shape[0], p * rows * count).view(np.uint64)
    out = np.zeros((x.shape[0], w), dtype=np.uint64)
    out -= d @ rev
    return out[0] if single else out


def pfks_literal(lwes, key, radix_log: int, count: int) -> list:
    """private_functional_keyswitch.rs:125-141 line by line on Python integers, for ONE output: lwes (p, n+1)"""
    lwes, key = np.asarray(lwes, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    p, rows = lwes.shape
    w = key.shape[3] * key.shape[4]
    output = [0] * w
    glevs = iter(key.reshape(p * rows, count, w))                            # let mut ksk_glevs = pfksk.glevs(..)
    for z in range(p):                                                       # for input in inputs.iter()
        for i in range(rows):                                                #   for i in 0..from_lwe.dim.0 + 1
            glev = next(glevs)                                               #     let glev = ksk_glevs.next().unwrap()
            decomp = radix_digits(int(lwes[z, i]), radix_log, count)         #     ScalarRadixIterator::new(ab[i], radix)
            # decomposed_scalar_glev_mad (glev_ciphertext_ops.rs:48-59): the GLWEs of the GLEV in reverse meet the digits in order
            for digit, glwe in zip(decomp, glev[::-1]):
                for c in range(w):
                    output[c] = (output[c] + digit * int(glwe[c])) & M64
    return [(-v) & M64 for v in output]                                      # glwe_negate_inplace


def uniform_case(seed, N, k, n, p, log, count, B, n_keys=1):
    """(keys (n_keys, p, n+1, count, k+1, N), lwes (B, p, n+1)), uniform words"""
    rng = np.random.default_rng([0xD0, seed, N, k, n, p, log, count, B, n_keys])
    return (rng.integers(0, 1 << 64, (n_keys, p, n + 1, count, k + 1, N), dtype=np.uint64),
            rng.integers(0, 1 << 64, (B, p, n + 1), dtype=np.uint64))


def extreme_case(seed, N, k, n, p, log, count, B):
    """inputs drawn from decomp_ref.extreme_words (every digit, hence every limb, at an end of its range) against a key of the
    PLANTED words (every byte plane at an end of its range), each word of each at least once where the shape has room"""
    rng = np.random.default_rng([0xD1, seed, N, k, n, p, log, count, B])
    words = np.array(extreme_words(log, count), dtype=np.uint64)
    lwes = words[rng.integers(0, words.size, (B, p, n + 1))]
    lwes.reshape(-1)[:min(words.size, lwes.size)] = words[:lwes.size]
    planted = np.array(PLANTED, dtype=np.uint64)
    key = planted[rng.integers(0, planted.size, (p, n + 1, count, k + 1, N))]
    key.reshape(-1)[:planted.size] = planted
    return key, lwes


# ---- honest keys, as generate_private_functional_keyswitch_key builds them (private_functional_keyswitch.rs:67-101)

def map_message_to_coefficient(N):
    """map 1: message z -> coefficient z"""
    def f(x):
        poly = np.zeros(N, dtype=np.uint64)
        poly[:len(x)] = x
        return poly
    return f


def map_times_minus_key_poly(s_poly):
    """generate_circuit_bootstrapping_pfks_keys (:160-183): *c = -x[0] * a over the coefficients a of one GLWE key polynomial"""
    s_poly = np.asarray(s_poly, dtype=np.uint64)
    return lambda x: (np.zeros(1, dtype=np.uint64) - np.asarray(x, dtype=np.uint64)[:1]) * s_poly


def map_to_constant(N):
    """the "b" GLEV (:192-195): coeffs[0] = x[0]"""
    def f(x):
        poly = np.zeros(N, dtype=np.uint64)
        poly[0] = x[0]
        return poly
    return f


def glwe_encrypt_constant_mask(rng, glwe_sk, msgs, noise_bound):
    """glwe_encrypt with constant mask polynomials a_i(X) = a_i: still a valid GLWE sample of msgs under glwe_sk (b = sum_i a_i
    s_i + m + e holds exactly), and a_i * s_i is a scaling instead of a negacyclic product: big keys in seconds"""
    msgs = np.asarray(msgs, dtype=np.uint64)
    m, N = msgs.shape
    sk = np.asarray(glwe_sk, dtype=np.uint64).reshape(-1, N)
    k = sk.shape[0]
    ct = np.zeros((m, k + 1, N), dtype=np.uint64)
    ct[:, :k, 0] = rng.integers(0, 1 << 64, (m, k), dtype=np.uint64)
    ct[:, k] = msgs + R.small_noise(rng, (m, N), noise_bound)
    for i in range(k):
        ct[:, k] += ct[:, i, :1] * sk[i][None, :]
    return ct


def honest_key(rng, lwe_sk, glwe_sk, N, p, radix_log, count, fmap, constant_mask=False):
    """row (z, i, lvl) = GLWE encryption of map(e_z * s_i * 2^(64 - log (lvl+1))), s_n = -1: (p, n+1, count, k+1, N)"""
    lwe_sk = np.asarray(lwe_sk, dtype=np.uint64)
    n = lwe_sk.size
    s = np.concatenate([lwe_sk, np.array([M64], dtype=np.uint64)])           # from_key.s() chained with minus_one
    msgs = np.zeros((p, n + 1, count, N), dtype=np.uint64)
    for z in range(p):
        for i in range(n + 1):
            for lvl in range(count):
                x = np.zeros(p, dtype=np.uint64)
                x[z] = s[i] << np.uint64(64 - radix_log * (lvl + 1))          # scale_by_decomposition_factor
                msgs[z, i, lvl] = fmap(x)
    enc = glwe_encrypt_constant_mask if constant_mask else R.glwe_encrypt
    k = np.asarray(glwe_sk).size // N
    return enc(rng, glwe_sk, msgs.reshape(-1, N), NOISE).reshape(p, n + 1, count, k + 1, N)


def cbs_pfks_keys(rng, lwe_sk, glwe_sk, N, radix_log, count, constant_mask=False):
    """generate_circuit_bootstrapping_pfks_keys (:145-207): k keys that multiply by -S_r, then the "b" key: (k+1, 1, n+1, count,
    k+1, N)"""
    sk = np.asarray(glwe_sk, dtype=np.uint64).reshape(-1, N)
    maps = [map_times_minus_key_poly(s_r) for s_r in sk] + [map_to_constant(N)]
    return np.stack([honest_key(rng, lwe_sk, glwe_sk, N, 1, radix_log, count, f, constant_mask) for f in maps])


def lwe_phases(lwes, lwe_sk) -> np.ndarray:
    lwes = np.asarray(lwes, dtype=np.uint64)
    return lwes[..., -1] - (lwes[..., :-1] * np.asarray(lwe_sk, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def meaning_bounds(n: int, p: int, count: int, log: int, weight: float = 1.0):
    """(bound where the map puts a phase, bound where it puts nothing), in units of the torus.  Derived, not measured.
    Rounding: each of the n + 1 words of an input (the body included: it is decomposed too) is replaced by its nearest multiple of
    2^(64 - count log), off by at most 2^-(count log + 1), and enters the phase times s_i in {0, 1} (the body: times 1), then
    through the map; `weight` bounds the map's gain on one input per output coefficient (1 for a coefficient that receives one
    input as it is or times a binary key coefficient).  Key noise: every one of the p (n+1) count key rows carries |e| <= NOISE in
    each coefficient, times a scalar digit of magnitude <= 2^(log - 1)."""
    noise = p * (n + 1) * count * 2.0 ** (log - 1) * NOISE / 2.0 ** 64
    return weight * (n + 1) * 2.0 ** -(count * log + 1) + noise, noise


def extract_and_rotate(glwes, l_cbs: int, log_cbs: int) -> np.ndarray:
    """`extract_and_rotate_lo_noise_glwe` (circuit_bootstrapping.rs:224-252): (B, k+1, N) -> (B, l_cbs, k N + 1).  Level i is
    `sample_extract`(i) (glwe_ciphertext_ops.rs:31-76: mask word p N + j is coefficient i - j of polynomial p for j <= i, minus
    coefficient i + N - j beyond) with 2^(64 - (log_cbs (i+1) + 1)) added to the body"""
    g = np.asarray(glwes, dtype=np.uint64)
    B, k1, N = g.shape
    k = k1 - 1
    out = np.empty((B, l_cbs, k * N + 1), dtype=np.uint64)
    j = np.arange(N)
    for i in range(l_cbs):
        idx = np.where(j <= i, i - j, i + N - j)
        vals = g[:, :k, idx]
        out[:, i, :k * N] = np.where(j <= i, vals, np.uint64(0) - vals).reshape(B, k * N)
        out[:, i, k * N] = g[:, k, i] + np.uint64(1 << (64 - (log_cbs * (i + 1) + 1)))
    return out
