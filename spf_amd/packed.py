"""The plaintext side of packed integers (`PackedDynamicGenericInt`, parasol_runtime/src/fluent/generic_int.rs:162-176): an
n-bit integer in one L1 GLWE, bit i (least significant first, `to_bits`, fluent/int.rs:47-49, uint.rs:30-32) in coefficient
X^i of the message polynomial at one plaintext bit.  Host only, no GPU; the ciphertext side is Engine.glwe_pack /
glwe_unpack_l1 / unpack_circuit_bootstrap."""
from __future__ import annotations

import numpy as np

from .params import DEFAULT_128, Params


def _check_bits(n_bits: int, params: Params):
    if not 0 < n_bits <= params.polynomial_degree:
        raise ValueError(f"n_bits must be in 1 ..= {params.polynomial_degree}, got {n_bits}")


def packed_plaintext(value: int, n_bits: int, params: Params = DEFAULT_128) -> np.ndarray:
    """the u64 message polynomial of `encode` (generic_int.rs:231-242): coefficient i = bit i of `value` for i < n_bits, in
    two's complement for a negative value, 0 above.  `value` must fit n_bits bits, signed (-2^(n-1) ..) or unsigned
    (.. 2^n - 1), as `assert_in_bounds` asks (int.rs:21-27, uint.rs:21-23)."""
    _check_bits(n_bits, params)
    value = int(value)
    if not -(1 << (n_bits - 1)) <= value < (1 << n_bits):
        raise ValueError(f"{value} does not fit in {n_bits} bits")
    v = value & ((1 << n_bits) - 1)
    out = np.zeros(params.polynomial_degree, dtype=np.uint64)
    out[:n_bits] = [(v >> i) & 1 for i in range(n_bits)]
    return out


def packed_decode(coeffs, n_bits: int, signed: bool) -> int:
    """`from_bits` of the first n_bits decoded coefficients (generic_int.rs:245-258): bit i is set where coefficient i is 1;
    signed values are sign-extended from bit n_bits - 1 (int.rs:29-45)."""
    c = np.asarray(coeffs, dtype=np.uint64).reshape(-1)
    if not 0 < n_bits <= c.size:
        raise ValueError(f"n_bits must be in 1 ..= {c.size}, got {n_bits}")
    v = sum(1 << i for i in range(n_bits) if int(c[i]) == 1)
    if signed and v >> (n_bits - 1):
        v -= 1 << n_bits
    return v


def trivial_packed_glwe(value: int, n_bits: int, params: Params = DEFAULT_128) -> np.ndarray:
    """`PackedDynamicGenericInt::trivial_encrypt` (generic_int.rs:270-280): zero mask, body coefficient i = bit i << 63 (the
    message at one plaintext bit); (k+1)*N words"""
    out = np.zeros(params.glwe_words, dtype=np.uint64)
    out[params.glwe_size * params.polynomial_degree:] = packed_plaintext(value, n_bits, params) << np.uint64(63)
    return out
