"""Shapes, inputs, generators and the reference of the plaintext polynomial linear maps over GLWE ciphertexts
(`glwe_polynomial_mad`, `glwe_scalar_mad`, `sub_glwe_ciphertexts`, `glwe_negate_inplace`, `glwe_rotate`: sunscreen_tfhe
ops/ciphertext/glwe_ciphertext_ops.rs:164-183, :189-202, :121-141, :147-156, :285-305), shared by
tests/test_glwe_poly_reference.py (CPU), tests/test_gpu_glwe_poly_linear.py and tests/test_gpu_glwe_poly_linear_cpp.py.
No GPU, no oracle and no library here: numpy on wrapping uint64.

K GLWEs x_k of k+1 polynomials of N words, an M x K matrix w of sparse plaintext polynomials and an optional bias of M plaintext
polynomials, in R = Z_2^64[X]/(X^N + 1):
    out_m[p] = sum_k w[m][k] * x_k[p]   for every polynomial p, mask then body;    out_m[k] += bias[m]
The matrix is held in CSR form over its M * K polynomials: (offsets [M K + 1], exponents [T], coefficients [T])."""
import os
import re

import numpy as np

from tests import poly_ref

U = np.uint64
M64 = (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
LDS, STREAM = "glwe_poly_lds_kernel", "glwe_poly_stream_kernel"
SLOTS, MAX_ROWS, MAX_TERMS, MAX_POLYS = 64, 4096, 1 << 24, 1 << 22
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spf_amd", "csrc")


def row_tile() -> int:
    """GLWE_POLY_VT, the output rows of one workgroup, read out of the source (as launch_slice_cases.constants reads its limits)"""
    with open(os.path.join(CSRC, "spf_glwe_poly.hpp")) as f:
        found = re.findall(r"constexpr int GLWE_POLY_VT = (\d+);", f.read())
    assert len(found) == 1, found
    return int(found[0])


# ---- the matrix -------------------------------------------------------------------------------------------------------------

def csr(polys, M: int, K: int):
    """polys[m][k] = a list of (exponent, coefficient) terms, in the order given, duplicates kept -> the CSR triple"""
    off, exp, coef = [0], [], []
    for m in range(M):
        for k in range(K):
            for e, c in polys[m][k]:
                exp.append(e)
                coef.append(c)
            off.append(len(exp))
    return np.array(off, dtype=np.uint32), np.array(exp, dtype=np.uint32), np.array(coef, dtype=np.int64)


def csr_of_dense(dense):
    """(M, K, N) int64 -> the CSR triple of its non-zeros, exponents ascending (what Engine.load_glwe_poly_weights keeps)"""
    d = np.asarray(dense, dtype=np.int64)
    M, K, _ = d.shape
    return csr([[[(int(e), int(d[m, k, e])) for e in np.nonzero(d[m, k])[0]] for k in range(K)] for m in range(M)], M, K)


def dense_of_csr(triple, M: int, K: int, N: int) -> np.ndarray:
    """the CSR triple as (M, K, N) wrapping uint64 coefficients, duplicates added"""
    off, exp, coef = triple
    d = np.zeros((M, K, N), dtype=np.uint64)
    for i in range(M * K):
        for t in range(int(off[i]), int(off[i + 1])):
            d[i // K, i % K, int(exp[t])] += U(int(coef[t]) & M64)
    return d


def is_constants_only(triple) -> bool:
    return not np.asarray(triple[1]).any()


def kernel_name(triple, forced=None) -> str:
    """the kernel a call on this slot must report under SPF_GLWE_POLY_PATH = forced (None: unset)"""
    return STREAM if is_constants_only(triple) and forced != "lds" else LDS


# term classes: how the exponents and the coefficients of one polynomial are drawn
def seam_exponents(N: int) -> list:
    """every exponent at which the rotated read changes its shape: none, one, the last, the half; at N = 2048 the thread stride"""
    return sorted({0, 1, N - 1, N // 2} | ({255, 256, 257} if N == 2048 else set()))


EXTREME_COEFFICIENTS = [INT64_MIN, -1, 0, 1, INT64_MAX]


def random_polys(seed, M, K, N, terms=3, cls="mixed", empty_every=0):
    """polys[m][k] for csr(): `terms` terms per polynomial.  cls: "mixed" exponents uniform below N and int64 coefficients;
    "seams" exponents from seam_exponents; "constants" exponent 0 only; "small" coefficients in [-8, 8].  Polynomial number i
    (row-major) is left empty where empty_every divides i + 1."""
    rng = np.random.default_rng([0xF0, seed, M, K, N, terms])
    seams = seam_exponents(N)
    out = []
    for m in range(M):
        row = []
        for k in range(K):
            if empty_every and (m * K + k + 1) % empty_every == 0:
                row.append([])
                continue
            poly = []
            for _ in range(terms):
                e = 0 if cls == "constants" else int(seams[rng.integers(len(seams))]) if cls == "seams" else int(rng.integers(N))
                c = int(rng.integers(-8, 9)) if cls == "small" else int(rng.integers(INT64_MIN, INT64_MAX, endpoint=True))
                poly.append((e, c))
            row.append(poly)
        out.append(row)
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def uniform_inputs(seed, B, K, k1, N) -> np.ndarray:
    return np.random.default_rng([0xF1, seed, B, K, k1, N]).integers(0, 1 << 64, (B, K, k1, N), dtype=np.uint64)


def extreme_inputs(B, K, k1, N) -> np.ndarray:
    """words that are all 0x00.. or all 0xff.., in a pattern no rotation maps onto itself"""
    j = np.arange(B * K * k1 * N)
    return np.where((j * j + j // 3) % 5 < 2, U(M64), U(0)).astype(np.uint64).reshape(B, K, k1, N)


def ones_inputs(B, K, k1, N) -> np.ndarray:
    return np.full((B, K, k1, N), M64, dtype=np.uint64)


def random_bias(seed, M, N) -> np.ndarray:
    return np.random.default_rng([0xF2, seed, M, N]).integers(0, 1 << 64, (M, N), dtype=np.uint64)


# ---- the reference ----------------------------------------------------------------------------------------------------------

def poly_linear_ref(x, triple, M: int, K: int, bias=None) -> np.ndarray:
    """from the definition, term by term: x (B, K, k+1, N) -> (B, M, k+1, N).  For every term c X^e of w[m][k]:
    acc_m += U(c) * mul_monomial(x[:, k], e) on wrapping uint64; then the bias on the body."""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    off, exp, coef = triple
    B, Kx, k1, N = x.shape
    assert Kx == K and len(off) == M * K + 1
    out = np.zeros((B, M, k1, N), dtype=np.uint64)
    for m in range(M):
        for k in range(K):
            for t in range(int(off[m * K + k]), int(off[m * K + k + 1])):
                out[:, m] += U(int(coef[t]) & M64) * poly_ref.mul_monomial(x[:, k], int(exp[t]))
    if bias is not None:
        out[:, :, k1 - 1] += np.asarray(bias, dtype=np.uint64)[None]
    return out
