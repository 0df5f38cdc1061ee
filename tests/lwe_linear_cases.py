"""Shapes, inputs, references and bounds of the plaintext linear maps over LWE ciphertexts (`scalar_mul_ciphertext_mad` then
`add_lwe_inplace`, sunscreen_tfhe ops/ciphertext/lwe_ciphertext_ops.rs:48-66, :4-18), shared by
tests/test_lwe_linear_reference.py (CPU) and tests/test_gpu_lwe_linear.py.  No GPU and no oracle here: numpy and Python integers.

K LWEs ct_k of W words (the body last), an M x K matrix w of int64 and an optional bias of M words:
    out_m[c] = sum_k (uint64)w[m][k] * ct_k[c]   for every word c, mod 2^64;    out_m[W-1] += bias[m]"""
import numpy as np

from tests.pfks_cases import PLANTED

M64 = (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
VALU = "lwe_linear_valu_kernel"
SEG_COLUMNS = 1023 * 128        # spf_pfks.hpp: columns between two folds of the GEMM's int32 accumulators


def limb_range(U: int):
    """weights w whose NEGATION has U balanced int8 limbs: -w = sum_u 256^u e_u, e_u in [-128, 127], reaches
    [-128 S, 127 S] with S = 1 + 256 + .. + 256^(U-1), so w is in [-127 S, 128 S]"""
    S = sum(256 ** u for u in range(U))
    return -127 * S, 128 * S


CLASS_RANGES = {U: limb_range(U) for U in (1, 2, 3)}
assert CLASS_RANGES == {1: (-127, 128), 2: (-32639, 32896), 3: (-8355711, 8421504)}
FIRST_BEYOND = (CLASS_RANGES[3][0] - 1, CLASS_RANGES[3][1] + 1)     # the first weights no class holds, on each side


def limbs_of(lo: int, hi: int) -> int:
    """the class of a matrix whose weights span [lo, hi]: the smallest U whose range holds both; 0: none (the VALU kernel)"""
    for U in (1, 2, 3):
        a, b = CLASS_RANGES[U]
        if a <= lo and hi <= b:
            return U
    return 0


def kernel_name(weights) -> str:
    """the product kernel of the matrix-core path for this matrix, or the VALU kernel's name where that path declines it"""
    w = np.asarray(weights, dtype=np.int64)
    U = limbs_of(int(w.min()), int(w.max()))
    return f"pfks_gemm_kernel<{U}>" if U else VALU


def balanced_limbs(d: int, U: int):
    """the split the limb kernel makes of d = -w: least significant first; None where U limbs do not hold d"""
    out = []
    for _ in range(U):
        e = ((d & 0xff) ^ 0x80) - 0x80
        out.append(e)
        d = (d - e) >> 8
    return out if d == 0 else None


def linear_ref(lwes, weights, bias=None) -> np.ndarray:
    """one wrapping uint64 matrix product: lwes (K, W) or (B, K, W), weights (M, K) int64 -> (M, W) or (B, M, W)"""
    x = np.asarray(lwes, dtype=np.uint64)
    w = np.asarray(weights, dtype=np.int64).view(np.uint64)
    single = x.ndim == 2
    x = x.reshape((-1,) + x.shape[-2:])
    out = np.stack([w @ xb for xb in x])
    if bias is not None:
        out[:, :, -1] += np.asarray(bias, dtype=np.uint64)[None, :]
    return out[0] if single else out


def linear_literal(lwes, weights, bias=None) -> list:
    """lwe_ciphertext_ops.rs line by line on Python integers, for ONE input vector: lwes (K, W) -> M lists of W words.
    `scalar_mul_ciphertext_mad` (:48-66): c[i] = c[i] + a[i] * scalar (wrapping) over the mask and the body;
    `add_lwe_inplace` (:4-18) is the `+=` of the same loop with the scalar 1.  The scalar is the weight as a torus word."""
    lwes = np.asarray(lwes, dtype=np.uint64)
    K, W = lwes.shape
    out = []
    for m, row in enumerate(np.asarray(weights, dtype=np.int64)):
        c = [0] * W                                                       # a zero (trivial) ciphertext
        for k in range(K):
            scalar = int(row[k]) & M64
            for i in range(W):                                            # a.iter().zip(c) over the mask, then the body
                c[i] = (c[i] + int(lwes[k, i]) * scalar) & M64
        if bias is not None:
            c[W - 1] = (c[W - 1] + int(bias[m])) & M64                    # a trivial encryption of the constant, added
        out.append(c)
    return out


def uniform_inputs(seed, B, K, W) -> np.ndarray:
    return np.random.default_rng([0xE0, seed, B, K, W]).integers(0, 1 << 64, (B, K, W), dtype=np.uint64)


def planted_inputs(seed, B, K, W) -> np.ndarray:
    """input words from PLANTED (every byte plane at an end of its range), each at least once where there is room"""
    rng = np.random.default_rng([0xE1, seed, B, K, W])
    planted = np.array(PLANTED, dtype=np.uint64)
    x = planted[rng.integers(0, planted.size, (B, K, W))]
    x.reshape(-1)[:min(planted.size, x.size)] = planted[:x.size]
    return x


def class_weights(seed, M, K, cls, plant=True) -> np.ndarray:
    """an (M, K) matrix of one class.  1, 2, 3: uniform over that class's range with its two end values planted (so that the
    matrix is of that class whatever was drawn); "beyond": class 3 with the first value past its upper end planted;
    "int64": uniform int64 with INT64_MIN, -1, 0 and INT64_MAX planted.  Planted values go to the front, then wherever they
    fit: a 1 x 1 matrix holds the upper end only."""
    rng = np.random.default_rng([0xE2, seed, M, K, {1: 1, 2: 2, 3: 3, "beyond": 4, "int64": 5, "ends": 6}[cls]])
    if cls == "int64":
        w = rng.integers(INT64_MIN, INT64_MAX, (M, K), dtype=np.int64, endpoint=True)
        ends = [INT64_MAX, INT64_MIN, -1, 0]
    elif cls == "beyond":
        lo, hi = CLASS_RANGES[3]
        w = rng.integers(lo, hi, (M, K), dtype=np.int64, endpoint=True)
        ends = [FIRST_BEYOND[1]]
    elif cls == "ends":                     # every weight at an end of a class: all limbs at an end of their range
        vals = np.array([v for U in (1, 2, 3) for v in CLASS_RANGES[U]], dtype=np.int64)
        w = vals[rng.integers(0, vals.size, (M, K))]
        ends = list(vals[::-1])
    else:
        lo, hi = CLASS_RANGES[cls]
        w = rng.integers(lo, hi, (M, K), dtype=np.int64, endpoint=True)
        ends = [hi, lo]
    if plant:
        flat = w.reshape(-1)
        flat[:min(len(ends), flat.size)] = ends[:flat.size]
    return w


def lwe_phases(lwes, lwe_sk) -> np.ndarray:
    lwes = np.asarray(lwes, dtype=np.uint64)
    return lwes[..., -1] - (lwes[..., :-1] * np.asarray(lwe_sk, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)
