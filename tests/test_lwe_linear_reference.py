"""The plaintext linear maps over LWE ciphertexts without a GPU: tests/lwe_linear_cases.py's `linear_ref` against the reference's
two functions restated line by line, the balanced limb split the matrix cores are fed with, and what the operation MEANS on
honest encryptions.  The GPU file compares words with `linear_ref`; this file is what makes `linear_ref` the reference."""
import os
import re

import numpy as np
import pytest

from tests import lwe_linear_cases as LC
from tests import poly_ref as R
from tests.pbs_graph_cases import SMALL16, TEST1
from tests.polyref_cases import NOISE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["spf_load_lwe_linear_weights", "spf_lwe_linear_batch", "spf_lwe_linear_enqueue", "spf_last_lwe_linear_kernel",
           "spf_group_load_lwe_linear_weights", "spf_group_lwe_linear_batch"]


@pytest.mark.parametrize("cls", [1, 2, 3, "beyond", "int64", "ends"])
@pytest.mark.parametrize("bias", ["null", "zero", "ones"])
def test_linear_ref_is_the_reference_line_by_line(cls, bias):
    M, K, W = 3, 5, 7
    w = LC.class_weights(1, M, K, cls)
    b = {"null": None, "zero": np.zeros(M, dtype=np.uint64), "ones": np.full(M, LC.M64, dtype=np.uint64)}[bias]
    for x in (LC.uniform_inputs(2, 2, K, W), LC.planted_inputs(3, 2, K, W)):
        got = LC.linear_ref(x, w, b)
        assert got.shape == (2, M, W) and got.dtype == np.uint64
        for i in range(2):
            assert got[i].tolist() == LC.linear_literal(x[i], w, b), (cls, bias, i)
        assert np.array_equal(LC.linear_ref(x[1], w, b), got[1])


def test_bias_changes_the_body_word_only():
    w, x = LC.class_weights(4, 4, 3, 2), LC.uniform_inputs(5, 2, 3, 9)
    plain = LC.linear_ref(x, w)
    assert np.array_equal(LC.linear_ref(x, w, np.zeros(4, dtype=np.uint64)), plain)
    full = LC.linear_ref(x, w, np.full(4, LC.M64, dtype=np.uint64))
    assert np.array_equal(full[..., :-1], plain[..., :-1])
    assert np.array_equal(full[..., -1], plain[..., -1] - np.uint64(1))


def test_the_balanced_limbs_recombine_to_minus_w_at_each_end_of_each_class():
    for U in (1, 2, 3):
        lo, hi = LC.CLASS_RANGES[U]
        for w in (lo, hi, lo + 1, hi - 1, 0, -1, 1):
            limbs = LC.balanced_limbs(-w, U)
            assert limbs is not None and len(limbs) == U, (U, w)
            assert all(-128 <= e <= 127 for e in limbs), (U, w, limbs)
            assert sum(e * 256 ** u for u, e in enumerate(limbs)) == -w, (U, w, limbs)
        assert LC.balanced_limbs(-lo, U) == [127] * U and LC.balanced_limbs(-hi, U) == [-128] * U
        # the first weight on each side that the class declines goes to the next class, or to none
        for w in (lo - 1, hi + 1):
            assert LC.balanced_limbs(-w, U) is None, (U, w)
            assert LC.limbs_of(w, w) == (U + 1 if U < 3 else 0), (U, w)
        assert LC.limbs_of(lo, hi) == U
    assert LC.limbs_of(0, 0) == 1
    for w in (LC.INT64_MIN, LC.INT64_MAX) + LC.FIRST_BEYOND:
        assert LC.limbs_of(w, w) == 0


def test_kernel_names_of_the_weight_classes():
    for cls, name in [(1, "pfks_gemm_kernel<1>"), (2, "pfks_gemm_kernel<2>"), (3, "pfks_gemm_kernel<3>"), ("ends", "pfks_gemm_kernel<3>"),
                      ("beyond", LC.VALU), ("int64", LC.VALU)]:
        assert LC.kernel_name(LC.class_weights(6, 3, 4, cls)) == name, cls


def test_the_int32_bound_of_the_accumulators():
    """|limb| <= 128 and |plane| <= 128: a segment of SEG_COLUMNS columns sums to at most SEG_COLUMNS * 2^14 < 2^31, and one more
    round of 128 columns would not fit"""
    assert LC.SEG_COLUMNS * (1 << 14) < (1 << 31) <= (LC.SEG_COLUMNS + 128) * (1 << 14)
    assert LC.balanced_limbs(-128, 1) == [-128]                          # the weight 128 is fed as the limb -128


@pytest.mark.parametrize("P,kind", [(SMALL16, 0), (SMALL16, 1), (TEST1, 0), (TEST1, 1)])
def test_meaning_on_honest_encryptions(P, kind):
    """messages m_k at Delta = 2^60 (four bits), |e_k| <= NOISE: the phase of output m is sum_k w[m][k] (m_k Delta + e_k) + bias[m]
    exactly, so it differs from sum_k w[m][k] m_k Delta + bias[m] by at most sum_k |w[m][k]| NOISE.  Derived, not measured."""
    n = P.lwe_n if kind == 0 else P.k * P.N
    rng = np.random.default_rng([0xE3, n, kind])
    sk = R.binary_key(rng, n)
    K, M, B, delta = 6, 4, 3, 1 << 60
    w = rng.integers(-9, 10, (M, K), dtype=np.int64)
    w[0] = [1 << 4, 1, 0, 0, 0, 0]                                        # the bivariate pack: left * 2^bits + right
    bias = rng.integers(0, 16, M, dtype=np.uint64) * np.uint64(delta)
    msgs = rng.integers(0, 16, (B, K))
    x = np.stack([[R.lwe_encrypt(rng, sk, int(m) * delta, NOISE) for m in row] for row in msgs])
    assert x.shape == (B, K, n + 1)
    phases = LC.lwe_phases(LC.linear_ref(x, w, bias), sk)
    for b in range(B):
        for m in range(M):
            want = (sum(int(w[m, k]) * int(msgs[b, k]) * delta for k in range(K)) + int(bias[m])) & LC.M64
            err = (int(phases[b, m]) - want) & LC.M64
            err = min(err, (1 << 64) - err)
            assert err <= int(np.abs(w[m]).sum()) * NOISE, (b, m, err)


def test_header_rust_block_and_integration_guide_name_the_exports():
    hdr = open(os.path.join(ROOT, "include", "spf_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "spf_hip.rs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert f"pub fn {name}(" in rust, name
        assert f"`{name}`" in guide, name
    assert "SPF_LWE_LINEAR_SLOTS = 64" in hdr and "pub const SPF_LWE_LINEAR_SLOTS:" in rust
    assert hdr.count("lwe_ciphertext_ops.rs:48-66, :4-18") >= 2           # at the context's entries and at the group's
    assert "weights: *const i64" in rust
    assert not re.search(r"spf_lwe_linear\w*_dev\b", hdr)


def test_the_binding_and_the_mirrors_have_the_methods():
    import spf_amd
    from spf_amd import _ffi
    names = {s[0] for s in _ffi.SYMBOLS}
    assert set(EXPORTS) <= names
    for cls in (spf_amd.Engine, spf_amd.Group):
        for meth in ("load_lwe_linear_weights", "lwe_linear", "lwe_linear_enqueue", "last_lwe_linear_kernel"):
            assert callable(getattr(cls, meth)), (cls, meth)
    assert _ffi.LWE_LINEAR_SLOTS == 64
    for meth in ("load_lwe_linear_weights", "lwe_linear"):
        assert callable(getattr(spf_amd.Evaluation, meth))
    mirror = open(os.path.join(ROOT, "include", "spf_evaluation.hpp")).read()
    assert "spf_group_load_lwe_linear_weights(" in mirror and "spf_group_lwe_linear_batch(" in mirror
