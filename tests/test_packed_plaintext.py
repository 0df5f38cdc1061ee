"""Packed integers on the host side: the plaintext helpers of spf_amd.packed against the reference's semantics
(`PackedDynamicGenericInt`, parasol_runtime fluent/generic_int.rs:162-280; `to_bits` / `from_bits`, fluent/int.rs:21-49,
uint.rs:21-32), and the closed form the pack kernel computes against the reference's construction restated with the oracle
(`DynamicGenericIntGraphNodes::pack`, fluent/dynamic_generic_int_graph_nodes.rs:139-200: `MulXN(i)` of bit i, then a
pairwise tree of `GlweAdd`s).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import _ffi
from tests.test_gpu_generic import TEST1, TEST2

M64 = (1 << 64) - 1


def closed_form_pack(bits, N: int, k: int) -> np.ndarray:
    """out[p*N + j] = sum_i s * bits[i][p*N + (j - i mod N)], s = -1 when j < i (X^i * bit_i mod X^N + 1), wrapping"""
    bits = np.asarray(bits, dtype=np.uint64).reshape(len(bits), k + 1, N)
    out = np.zeros((k + 1, N), dtype=np.uint64)
    for i, x in enumerate(bits):
        r = np.roll(x, i, axis=1)
        r[:, :i] = np.uint64(0) - r[:, :i]
        out += r
    return out.reshape(-1)


def oracle_tree_pack(bits, N: int, k: int) -> np.ndarray:
    """dynamic_generic_int_graph_nodes.rs:139-200 with the oracle's KeylessEvaluation ops: bit 0 as is, bit i > 0 through
    MulXN(i); then ceil(log2 n) rounds of pairwise GlweAdd over chunks of two, an odd last one passed through"""
    n = len(bits)
    red = [bits[0]] + [O.glwe_mul_xn(bits[i], i, N, k) for i in range(1, n)]
    for _ in range((n - 1).bit_length()):          # next_power_of_two(n).ilog2()
        assert len(red) > 1
        red = [O.glwe_xor(c[0], c[1], N, k) if len(c) == 2 else c[0] for c in (red[j:j + 2] for j in range(0, len(red), 2))]
    assert len(red) == 1
    return red[0]


def _decode_bits(phase) -> np.ndarray:
    return np.array([O.decode(int(t), 1) for t in phase], dtype=np.uint64)


@pytest.mark.parametrize("value,n,signed", [(-42, 16, True), (-42, 15, True), (42, 16, False), (0xBEEF, 16, False),
                                             (1, 1, False), (0, 1, False), (-1, 1, True), (-1, 64, True),
                                             ((1 << 64) - 1, 64, False), (-(1 << 15), 16, True), ((1 << 15) - 1, 16, True)])
def test_packed_plaintext_round_trips(value, n, signed):
    P = spf_amd.DEFAULT_128
    pt = spf_amd.packed_plaintext(value, n, P)
    assert pt.shape == (P.polynomial_degree,) and pt.dtype == np.uint64
    want = [((value & ((1 << n) - 1)) >> i) & 1 for i in range(n)]
    assert pt[:n].tolist() == want and not pt[n:].any()
    assert spf_amd.packed_decode(pt, n, signed) == value
    g = spf_amd.trivial_packed_glwe(value, n, P)
    assert g.shape == (P.glwe_words,) and not g[:P.polynomial_degree].any()
    assert np.array_equal(g[P.polynomial_degree:], pt << np.uint64(63))
    assert spf_amd.packed_decode(_decode_bits(g[P.polynomial_degree:]), n, signed) == value


def test_packed_plaintext_at_n_equal_to_N_and_generic_shapes():
    N = 2048
    rng = np.random.default_rng(0x9AC0)
    v = int.from_bytes(rng.bytes(N // 8), "little")
    pt = spf_amd.packed_plaintext(v, N)
    assert spf_amd.packed_decode(pt, N, False) == v
    assert spf_amd.packed_decode(spf_amd.packed_plaintext(v - (1 << N) if v >> (N - 1) else v, N), N, True) == \
        (v - (1 << N) if v >> (N - 1) else v)
    P = spf_amd.DEFAULT_128.replace(polynomial_degree=128, glwe_size=2)
    g = spf_amd.trivial_packed_glwe(-42, 15, P)
    assert g.shape == (3 * 128,) and not g[:256].any()
    assert spf_amd.packed_decode(_decode_bits(g[256:]), 15, True) == -42


@pytest.mark.parametrize("value,n", [(1 << 16, 16), (-(1 << 15) - 1, 16), (2, 1), (-2, 1), (1 << 2048, 2048)])
def test_packed_plaintext_rejects_values_that_do_not_fit(value, n):
    with pytest.raises(ValueError):
        spf_amd.packed_plaintext(value, n)
    with pytest.raises(ValueError):
        spf_amd.trivial_packed_glwe(value, n)


@pytest.mark.parametrize("n", [0, -1, 2049])
def test_packed_plaintext_rejects_bit_counts_outside_1_to_N(n):
    with pytest.raises(ValueError):
        spf_amd.packed_plaintext(0, n)
    with pytest.raises(ValueError):
        spf_amd.packed_decode(np.zeros(2048, dtype=np.uint64), n, False)
    with pytest.raises(ValueError):
        spf_amd.trivial_packed_glwe(0, n)


@pytest.mark.parametrize("OP", [O.DEFAULT_128, TEST1, TEST2], ids=["N2048k1", "N128k2", "N256k3"])
def test_closed_form_pack_equals_the_reference_tree(OP):
    rng = np.random.default_rng(0x9AC1 + OP.N)
    for n in (1, 2, 3, 15, 16, 17, 64 if OP.N > 128 else 128):
        bits = rng.integers(0, 1 << 64, size=(n, OP.glwe_len), dtype=np.uint64)
        if n > 2:
            bits[1] = 0
            bits[2] = M64
        assert np.array_equal(closed_form_pack(bits, OP.N, OP.k), oracle_tree_pack(bits, OP.N, OP.k)), n


def test_encrypted_packed_plaintext_decrypts_to_the_value():
    OP = O.DEFAULT_128
    rng = O.Rng(0x9AC2)
    sk = O.gen_binary_key(rng, OP.k * OP.N)
    for value, n, signed in [(-42, 16, True), (-42, 15, True), (40000, 16, False)]:
        msg = spf_amd.packed_plaintext(value, n) << np.uint64(63)
        ct = O.encrypt_glwe(rng, sk, msg, OP.N, OP.k, OP.glwe_std)
        assert spf_amd.packed_decode(_decode_bits(O.decrypt_glwe_raw(ct, sk, OP.N, OP.k)), n, signed) == value


def test_packed_entry_points_validate_before_touching_a_device():
    """null context / group: status 1 and a message, whatever the other arguments (no device is needed to say so)"""
    lib = _ffi.load_library()
    x = np.zeros(8, dtype=np.uint64)
    p = x.ctypes.data_as(C.c_void_p)
    for B, n in [(1, 16), (0, 16), (1, 0), (1, 4096), (1 << 40, 1 << 20)]:
        assert lib.spf_glwe_pack_batch(None, B, n, p, p) == 1
        assert lib.spf_glwe_unpack_l1_batch(None, B, n, p, p) == 1
        assert lib.spf_unpack_circuit_bootstrap_batch(None, B, n, p, p) == 1
        assert lib.spf_glwe_pack_dev(None, None, B, n, p, p) == 1
        assert lib.spf_glwe_unpack_l1_dev(None, None, B, n, p, p) == 1
        assert lib.spf_unpack_circuit_bootstrap_dev(None, None, B, n, p, p) == 1
        assert b"null" in lib.spf_last_error(None)
        assert lib.spf_group_glwe_pack_batch(None, B, n, p, p) == 1
        assert lib.spf_group_glwe_unpack_l1_batch(None, B, n, p, p) == 1
        assert lib.spf_group_unpack_circuit_bootstrap_batch(None, B, n, p, p) == 1
