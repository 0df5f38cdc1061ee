"""The reference of the plaintext polynomial linear maps over GLWE ciphertexts (tests/glwe_poly_cases.py's `poly_linear_ref`)
against independent statements of the same arithmetic, on the CPU: the Toeplitz product and the schoolbook product of
tests/poly_ref.py for dense weights, the reference's five functions as special cases, and decryption."""
import numpy as np
import pytest

from tests import glwe_poly_cases as GC
from tests import poly_ref

U = np.uint64


def dense_weights(seed, M, K, N):
    return np.random.default_rng([0xF3, seed, M, K, N]).integers(GC.INT64_MIN, GC.INT64_MAX, (M, K, N), dtype=np.int64, endpoint=True)


@pytest.mark.parametrize("N,M,K,B", [(16, 3, 2, 2), (128, 2, 3, 2), (2048, 1, 2, 1)])
def test_dense_weights_equal_the_toeplitz_product(N, M, K, B):
    k1 = 2
    d = dense_weights(1, M, K, N)
    x = GC.uniform_inputs(2, B, K, k1, N)
    bias = GC.random_bias(3, M, N)
    got = GC.poly_linear_ref(x, GC.csr_of_dense(d), M, K, bias)
    want = np.zeros((B, M, k1, N), dtype=np.uint64)
    for m in range(M):
        for k in range(K):
            want[:, m] += poly_ref.negacyclic_mul(x[:, k].reshape(B * k1, N), d[m, k].view(np.uint64)).reshape(B, k1, N)
    want[:, :, k1 - 1] += bias[None]
    assert np.array_equal(got, want)
    assert np.array_equal(GC.dense_of_csr(GC.csr_of_dense(d), M, K, N), d.view(np.uint64))


def test_dense_weights_equal_the_schoolbook_product_at_16():
    N, k1 = 16, 2
    d = dense_weights(4, 1, 1, N)
    x = GC.uniform_inputs(5, 1, 1, k1, N)
    got = GC.poly_linear_ref(x, GC.csr_of_dense(d), 1, 1)
    for p in range(k1):
        want = poly_ref.schoolbook_mul([int(v) for v in x[0, 0, p]], [int(v) & GC.M64 for v in d[0, 0]])
        assert [int(v) for v in got[0, 0, p]] == [int(v) & GC.M64 for v in want], p


def test_the_five_reference_functions_are_special_cases():
    N, k1, B = 128, 3, 2
    x = GC.uniform_inputs(6, B, 2, k1, N)
    # sub_glwe_ciphertexts: weights (1, -1)
    sub = GC.poly_linear_ref(x, GC.csr([[[(0, 1)], [(0, -1)]]], 1, 2), 1, 2)
    assert np.array_equal(sub[:, 0], x[:, 0] - x[:, 1])
    # glwe_negate_inplace: -1
    neg = GC.poly_linear_ref(x[:, :1], GC.csr([[[(0, -1)]]], 1, 1), 1, 1)
    assert np.array_equal(neg[:, 0], U(0) - x[:, 0])
    # glwe_scalar_mad: c + scalar * a
    mad = GC.poly_linear_ref(x, GC.csr([[[(0, 1)], [(0, -77)]]], 1, 2), 1, 2)
    assert np.array_equal(mad[:, 0], x[:, 0] + U(-77 & GC.M64) * x[:, 1])
    # a monomial X^e equals mul_monomial
    for e in GC.seam_exponents(N):
        rot = GC.poly_linear_ref(x[:, :1], GC.csr([[[(e, 1)]]], 1, 1), 1, 1)
        assert np.array_equal(rot[:, 0], poly_ref.mul_monomial(x[:, 0], e)), e
    # glwe_rotate: a plaintext constant added to the body, here through the bias with the identity weight
    bias = np.zeros((1, N), dtype=np.uint64)
    bias[0, 0] = U(1 << 62)
    rot = GC.poly_linear_ref(x[:, :1], GC.csr([[[(0, 1)]]], 1, 1), 1, 1, bias)
    want = x[:, 0].copy()
    want[:, k1 - 1, 0] += U(1 << 62)
    assert np.array_equal(rot[:, 0], want)
    # duplicate exponents add; an empty polynomial is zero
    dup = GC.poly_linear_ref(x, GC.csr([[[(5, 3), (5, 4), (5, -1)], []]], 1, 2), 1, 2)
    assert np.array_equal(dup[:, 0], U(6) * poly_ref.mul_monomial(x[:, 0], 5))
    assert not GC.poly_linear_ref(x, GC.csr([[[], []]], 1, 2), 1, 2).any()


def test_the_classification_and_the_kernel_names():
    assert GC.kernel_name(GC.csr([[[(0, 5)], []]], 1, 2)) == GC.STREAM
    assert GC.kernel_name(GC.csr([[[(0, 5)], []]], 1, 2), "lds") == GC.LDS
    assert GC.kernel_name(GC.csr([[[], []]], 1, 2)) == GC.STREAM
    assert GC.kernel_name(GC.csr([[[(0, 5)], [(1, 0)]]], 1, 2), "stream") == GC.LDS
    assert GC.row_tile() >= 2


def test_decryption_of_the_map_is_the_plaintext_product():
    """packed messages m_k in the top bits, noise |e| <= E: the phase of out_m is sum_k w[m][k] * (m_k + e_k) exactly, so it is
    within E * ||w[m]||_1 of the plaintext product sum_k w[m][k] * m_k + bias[m] on every coefficient"""
    N, k, K, M, E = 128, 2, 3, 2, 1 << 20
    rng = np.random.default_rng(0xF4)
    sk = poly_ref.binary_key(rng, k * N)
    msgs = rng.integers(0, 16, (K, N), dtype=np.uint64) << U(60)
    x = poly_ref.glwe_encrypt(rng, sk, msgs, E)[None]                     # (1, K, k+1, N)
    polys = GC.random_polys(7, M, K, N, terms=4, cls="small")
    triple = GC.csr(polys, M, K)
    bias = (rng.integers(0, 16, (M, N), dtype=np.uint64) << U(60))
    out = GC.poly_linear_ref(x, triple, M, K, bias)
    phase = poly_ref.glwe_phase(out[0], sk)                               # (M, N)
    plain = GC.poly_linear_ref(msgs[None, :, None, :], triple, M, K, bias)[0, :, 0]
    for m in range(M):
        norm1 = sum(abs(c) for k_ in range(K) for _, c in polys[m][k_])
        err = np.abs((phase[m] - plain[m]).view(np.int64))
        assert int(err.max()) <= E * norm1, (m, int(err.max()), E * norm1)
        assert err.any()                                                  # (there is noise: the bound is not vacuous)
