"""The plaintext side of packed integers (`PackedDynamicGenericInt`, parasol_runtime/src/fluent/generic_int.rs:162-176): an
n-bit integer in one L1 GLWE, bit i (least significant first, `to_bits`, fluent/int.rs:47-49, uint.rs:30-32) in coefficient
X^i of the message polynomial at one plaintext bit.  Host only, no GPU; the ciphertext side is Engine.glwe_pack /
glwe_unpack_l1 / unpack_circuit_bootstrap, and Engine.blind_rotation for the packed tables.  The strided layout of
Engine.lwe_ring_pack (message j at coefficient j * N / p) is at the end of this file."""
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


def table_plaintext(values, entry_bits: int, params: Params = DEFAULT_128):
    """A table of `entry_bits`-bit entries in one message polynomial, for Engine.blind_rotation: bit j of entry t at
    coefficient t * S + j, S the smallest power of two >= entry_bits.  Returns (coefficients, log_stride) with
    log_stride = log2 S.  len(values) * S <= N, and every value fits entry_bits bits as packed_plaintext asks.

    Rotating by an encrypted index t with this log_stride multiplies by X^-(t * S): coefficients 0 .. entry_bits-1 then hold
    entry t.  The coefficients above them hold the OTHER entries (those below t come back negated), so the result is meant for
    glwe_unpack_l1(.., entry_bits) and is no operand of glwe_pack, which expects zeros above its bits."""
    _check_bits(entry_bits, params)
    log_stride = (entry_bits - 1).bit_length()
    S = 1 << log_stride
    values = [int(v) for v in values]
    if len(values) * S > params.polynomial_degree:
        raise ValueError(f"{len(values)} entries of stride {S} do not fit {params.polynomial_degree} coefficients")
    out = np.zeros(params.polynomial_degree, dtype=np.uint64)
    for t, v in enumerate(values):
        out[t * S:t * S + entry_bits] = packed_plaintext(v, entry_bits, params)[:entry_bits]
    return out, log_stride


def trivial_table_glwe(values, entry_bits: int, params: Params = DEFAULT_128):
    """the zero-mask GLWE of table_plaintext at one plaintext bit (body coefficient = bit << 63), as trivial_packed_glwe is
    of packed_plaintext: ((k+1)*N words, log_stride).  See table_plaintext for what the rotated table may be used for."""
    coeffs, log_stride = table_plaintext(values, entry_bits, params)
    out = np.zeros(params.glwe_words, dtype=np.uint64)
    out[params.glwe_size * params.polynomial_degree:] = coeffs << np.uint64(63)
    return out, log_stride


# ---- the strided layout of ring packing (Engine.lwe_ring_pack, spf_lwe_ring_pack_batch) ----------------------------------------

def strided_positions(p: int, params: Params = DEFAULT_128) -> np.ndarray:
    """the coefficients j * N / p, j < p, that hold the p messages of a ring-packed GLWE (p a power of two <= N); every other
    coefficient of its phase holds 0.  They are the indices of sample_extract_l1_each, and log2(N / p) is the log_stride of
    Engine.blind_rotation."""
    N = params.polynomial_degree
    p = int(p)
    if p < 1 or p > N or p & (p - 1):
        raise ValueError(f"p must be a power of two in 1 ..= {N}, got {p}")
    return np.arange(p, dtype=np.int64) * (N // p)


def strided_plaintext(messages, params: Params = DEFAULT_128) -> np.ndarray:
    """the u64 message polynomial with messages[j] (torus words, taken mod 2^64) at coefficient j * N / p, p = len(messages)"""
    m = [int(v) & 0xFFFFFFFFFFFFFFFF for v in messages]
    out = np.zeros(params.polynomial_degree, dtype=np.uint64)
    out[strided_positions(len(m), params)] = np.array(m, dtype=np.uint64)
    return out


def strided_decode(coeffs, p: int, params: Params = DEFAULT_128) -> np.ndarray:
    """the p messages of a decoded (or raw) coefficient vector of N entries laid out by strided_plaintext"""
    c = np.asarray(coeffs).reshape(-1)
    if c.size != params.polynomial_degree:
        raise ValueError(f"expected {params.polynomial_degree} coefficients, got {c.size}")
    return c[strided_positions(p, params)]
