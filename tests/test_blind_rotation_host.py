"""The host side of blind rotation by an encrypted shift (`blind_rotation`, sunscreen_tfhe ops/bootstrapping/blind_rotation.rs:
202-223): the packed tables of spf_amd.packed that Engine.blind_rotation indexes, and the argument checks of the entry points
that need no device.  The GPU side is tests/test_gpu_blind_rotation.py."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import _ffi
from spf_amd.packed import table_plaintext, trivial_table_glwe

P = spf_amd.DEFAULT_128
N = P.polynomial_degree


@pytest.mark.parametrize("entry_bits,stride", [(1, 1), (3, 4), (8, 8)])
def test_table_layout_and_stride_rounding(entry_bits, stride):
    rng = np.random.default_rng(entry_bits)
    values = [int(v) for v in rng.integers(0, 1 << entry_bits, size=5)]
    values[0], values[1] = (1 << entry_bits) - 1, 0
    coeffs, log_stride = table_plaintext(values, entry_bits)
    assert 1 << log_stride == stride and coeffs.dtype == np.uint64 and coeffs.shape == (N,)
    exp = np.zeros(N, dtype=np.uint64)
    for t, v in enumerate(values):
        for j in range(entry_bits):
            exp[t * stride + j] = (v >> j) & 1
    assert np.array_equal(coeffs, exp)          # bit j of entry t at t * S + j, zeros in the padding and behind the table
    glwe, ls = trivial_table_glwe(values, entry_bits)
    assert ls == log_stride and glwe.shape == (P.glwe_words,) and glwe.dtype == np.uint64
    assert not glwe[:P.glwe_size * N].any()     # zero mask
    assert np.array_equal(glwe[P.glwe_size * N:], exp << np.uint64(63))


def test_table_fills_the_polynomial_and_refuses_more():
    assert table_plaintext([1] * N, 1)[1] == 0
    assert table_plaintext([5] * (N // 4), 3)[0].sum() == 2 * (N // 4)
    for values, bits in [([1] * (N + 1), 1), ([0] * (N // 4 + 1), 3), ([0] * (N // 8 + 1), 5), ([0], N + 1), ([0], 0)]:
        with pytest.raises(ValueError):
            table_plaintext(values, bits)
        with pytest.raises(ValueError):
            trivial_table_glwe(values, bits)
    with pytest.raises(ValueError):
        table_plaintext([8], 3)                 # an entry that does not fit its bits


@pytest.mark.parametrize("entry_bits,count", [(8, 16), (3, 512), (1, 2048)])
def test_rotation_by_t_strides_selects_entry_t(entry_bits, count):
    """X^-(t * S) (`rotate_glwe_negative_monomial_negacyclic`, the oracle's poly_mul_neg_monomial) brings entry t to
    coefficients 0 .. entry_bits-1: the first and the last t"""
    rng = np.random.default_rng(100 + entry_bits)
    values = [int(v) for v in rng.integers(0, 1 << entry_bits, size=count)]
    coeffs, log_stride = table_plaintext(values, entry_bits)
    for t in (0, count - 1):
        rot = O.poly_mul_neg_monomial(coeffs, t << log_stride)
        assert spf_amd.packed_decode(rot[:entry_bits], entry_bits, signed=False) == values[t], t


def test_entry_points_refuse_a_null_context_without_a_device():
    lib = _ffi.load_library()
    x = np.zeros(8, dtype=np.uint64)
    p = x.ctypes.data_as(C.c_void_p)
    for B, n, ls in [(1, 11, 0), (0, 4, 3), (1, 0, 0), (1, 12, 0), (1 << 40, 11, 0)]:
        assert lib.spf_blind_rotation_batch(None, B, n, ls, p, p, p) == 1
        assert b"null" in lib.spf_last_error(None)
        assert lib.spf_blind_rotation_dev(None, None, B, n, ls, p, p, p) == 1
        assert lib.spf_group_blind_rotation_batch(None, B, n, ls, p, p, p) == 1
        assert b"null" in lib.spf_last_error(None)
