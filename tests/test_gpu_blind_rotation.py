"""Blind rotation by an encrypted shift (`blind_rotation`, sunscreen_tfhe ops/bootstrapping/blind_rotation.rs:202-223) on the GPU:
one CMUX per bit whose high operand is a rotated read of the low one.  No tolerance anywhere: the words are those of the same
loop written with the existing mul_xn and cmux calls, hence the oracle's."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd.packed import trivial_table_glwe
from tests.util import random_glwe, to_engine_params

pytestmark = pytest.mark.gpu
P = O.DEFAULT_128.replace(lwe_n=1)
# test_gpu_generic.py's TEST1 (high_level.rs:9-58): N 128, k 2, 3 x 4 bits
TEST1 = O.DEFAULT_128.replace(lwe_n=128, lwe_std=1e-16, N=128, k=2, glwe_std=1e-16, pbs_radix_log=4, pbs_count=3,
                              cbs_radix_log=4, cbs_count=3, ks_radix_log=4, ks_count=3)
FOUR_WAVE, PER_WG, STREAM = "cmux4_kernel<4,4,rot>", "cmux_kernel<4,4,2,rot>", "cmux_kernel<4,4,2,stream,rot>"


@pytest.fixture(scope="module")
def eng():
    e = spf_amd.Engine(to_engine_params(P))
    yield e
    e.close()


def _shift(seed, B, n_bits, Q=P):
    """random complex values at 2^58, as test_gpu_keyless_ops.py's _ggsw: (B, n_bits, selector)"""
    r = np.random.default_rng(seed)
    out = np.empty((B, n_bits, Q.cbs_ggsw_fft_len), dtype=np.complex128)
    v = out.view(np.float64)
    v[...] = r.standard_normal(v.shape)
    v *= 2.0 ** 58
    return out


def oracle_loop(glwe, shift, log_stride, Q=P):
    """the issue's loop for one item, with the oracle's glwe_mul_xn (X^-r = X^(2N - r)) and cmux"""
    acc = glwe
    for i in range(shift.shape[0]):
        high = O.glwe_mul_xn(acc, 2 * Q.N - (1 << (i + log_stride)), Q.N, Q.k)
        acc = O.cmux(acc, high, shift[i], Q.N, Q.k, Q.cbs_radix_log, Q.cbs_count)
    return acc


def composed_loop(eng, glwe, shift, log_stride):
    """the same loop over the whole batch through the existing entry points"""
    acc = glwe
    for i in range(shift.shape[1]):
        high = eng.glwe_mul_xn(acc, 2 * P.N - (1 << (i + log_stride)))
        acc = eng.cmux(np.ascontiguousarray(shift[:, i]), acc, high)
    return acc


def test_parity_with_the_oracle_full_shift(eng):
    B, n_bits = 3, 11
    shift, glwe = _shift(41, B, n_bits), random_glwe(42, B, P.glwe_len)
    got = eng.blind_rotation(shift, glwe)
    assert eng.last_cmux_kernel() == FOUR_WAVE
    for b in range(B):
        assert np.array_equal(got[b], oracle_loop(glwe[b], shift[b], 0)), b


@pytest.mark.parametrize("B,n_bits,log_stride,kernel", [
    (1, 1, 0, FOUR_WAVE),
    (1, 1, 10, FOUR_WAVE),      # rotation by N/2
    (256, 2, 3, FOUR_WAVE),     # last batch size of the four-wave shape
    (257, 2, 0, PER_WG),        # ragged last workgroup
    (301, 3, 8, PER_WG),        # largest sum allowed: 3 + 8 = 11
    (896, 1, 5, STREAM),        # 896 selectors of 256 KiB = 224 MiB
])
def test_every_batch_shape_and_ping_pong_parity(eng, B, n_bits, log_stride, kernel):
    shift, glwe = _shift(1000 + B, B, n_bits), random_glwe(2000 + B + log_stride, B, P.glwe_len)
    assert shift.nbytes < 240e6
    before = glwe.copy()
    got = eng.blind_rotation(shift, glwe, log_stride)
    assert eng.last_cmux_kernel() == kernel
    assert np.array_equal(glwe, before)
    assert np.array_equal(got, composed_loop(eng, glwe, shift, log_stride))
    items = sorted({0, B - 2, B - 1} | {int(x) for x in np.linspace(1, B - 3, 5)} if B > 8 else set(range(B)))
    for b in items:
        assert np.array_equal(got[b], oracle_loop(glwe[b], shift[b], log_stride)), b


def test_dev_form_leaves_its_input_and_writes_the_output_for_either_parity(eng):
    """the device-pointer form: n_bits 1 (no intermediate), 2 and 3 (either ping-pong parity) into the caller's buffer"""
    B = 2
    glwe = random_glwe(77, B, P.glwe_len)
    d_in, d_out = eng.device_alloc(glwe.nbytes), eng.device_alloc(glwe.nbytes)
    try:
        eng.device_upload(d_in, glwe)
        for n_bits in (1, 2, 3):
            shift = _shift(70 + n_bits, B, n_bits)
            d_shift = eng.device_alloc(shift.nbytes)
            try:
                eng.device_upload(d_shift, shift)
                eng.blind_rotation_dev(None, B, n_bits, 1, d_shift, d_in, d_out)
                got, back = np.empty_like(glwe), np.empty_like(glwe)
                eng.device_download(None, got, d_out)
                eng.device_download(None, back, d_in)
            finally:
                eng.device_free(d_shift)
            assert np.array_equal(back, glwe)
            for b in range(B):
                assert np.array_equal(got[b], oracle_loop(glwe[b], shift[b], 1)), (n_bits, b)
        with pytest.raises(spf_amd.SpfError, match="overlaps"):
            eng.blind_rotation_dev(None, B, 1, 0, d_out, d_in, d_in)
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)


def _encrypted_bits(rng, sk, values, n_bits, Q=P):
    return np.stack([np.stack([O.encrypt_ggsw_fft(rng, sk, (s >> i) & 1, Q.N, Q.k, Q.cbs_radix_log, Q.cbs_count, Q.glwe_std)
                               for i in range(n_bits)]) for s in values])


def test_it_rotates(eng):
    """real ciphertexts: a message at 4 plaintext bits (a negated coefficient decodes differently), the shift's bits as GGSWs"""
    rng = O.Rng(0xB11D)
    sk = O.gen_binary_key(rng, P.k * P.N)
    msg = np.random.default_rng(3).integers(0, 16, P.N)
    enc = np.array([O.encode(int(v), 4) for v in msg], dtype=np.uint64)
    shifts = [0, 1, 1365, 2047]
    glwe = np.stack([O.encrypt_glwe(rng, sk, enc, P.N, P.k, P.glwe_std) for _ in shifts])
    got = eng.blind_rotation(_encrypted_bits(rng, sk, shifts, 11), glwe)
    for b, s in enumerate(shifts):
        dec = [O.decode(int(t), 4) for t in O.decrypt_glwe_raw(got[b], sk, P.N, P.k)]
        exp = [O.decode(int(t), 4) for t in O.poly_mul_neg_monomial(enc, s)]
        assert dec == exp, s


def test_table_lookup_end_to_end(eng):
    """array[i] with encrypted i: 16 entries of 8 bits, every index in one batch, the selected entry unpacked and decrypted"""
    rng = O.Rng(0x7AB1E)
    sk = O.gen_binary_key(rng, P.k * P.N)   # k = 1: the GLWE key is the flattened L1 LWE key
    entries = [int(v) for v in np.random.default_rng(8).integers(0, 256, 16)]
    table, log_stride = trivial_table_glwe(entries, 8, eng.params)
    assert log_stride == 3
    idx = list(range(16))
    out = eng.blind_rotation(_encrypted_bits(rng, sk, idx, 4), np.tile(table, (16, 1)), log_stride)
    lwe = eng.glwe_unpack_l1(out, 8)
    for i in idx:
        bits = [O.decode(O.decrypt_lwe_raw(lwe[i, j], sk), 1) for j in range(8)]
        assert spf_amd.packed_decode(bits, 8, signed=False) == entries[i], i


def test_generic_context_runs_the_composed_steps():
    Q = TEST1
    e = spf_amd.Engine(to_engine_params(Q))
    rng = O.Rng(0x6E4)
    sk = O.gen_binary_key(rng, Q.k * Q.N)
    B, n_bits = 3, 7
    shift = _encrypted_bits(rng, sk, [0, 85, 127], n_bits, Q)
    glwe = random_glwe(61, B, Q.glwe_len)
    got = e.blind_rotation(shift, glwe)
    assert e.last_cmux_kernel() == "generic_cmux_kernel"
    for b in range(B):
        assert np.array_equal(got[b], oracle_loop(glwe[b], shift[b], 0, Q)), b
    got = e.blind_rotation(shift[:, :2], glwe, 5)          # 2 + 5 = log2 N
    for b in range(B):
        assert np.array_equal(got[b], oracle_loop(glwe[b], shift[b, :2], 5, Q)), b
    e.close()


def test_group_returns_the_single_context_words(eng):
    B, n_bits, log_stride = 5, 2, 4
    shift, glwe = _shift(91, B, n_bits), random_glwe(92, B, P.glwe_len)
    grp = spf_amd.Group(to_engine_params(P), devices=[0, 0])
    try:
        got = grp.blind_rotation(shift, glwe, log_stride)
    finally:
        grp.close()
    assert np.array_equal(got, eng.blind_rotation(shift, glwe, log_stride))


def test_errors_leave_the_context_usable(eng):
    shift, glwe = _shift(95, 1, 2), random_glwe(96, 1, P.glwe_len)
    good = eng.blind_rotation(shift, glwe, 1)

    def refused(call, word):
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == 1 and word in str(e.value), str(e.value)
        assert np.array_equal(eng.blind_rotation(shift, glwe, 1), good)

    refused(lambda: eng.blind_rotation(shift[:, :0], glwe), "n_bits")
    refused(lambda: eng.blind_rotation(shift, glwe, 10), "log_stride")          # 2 + 10 = 12
    p = glwe.ctypes.data_as(C.c_void_p)
    refused(lambda: eng._ck(eng._lib.spf_blind_rotation_batch(eng._h, 1, 2, 0, None, p, p)), "null")
    refused(lambda: eng._ck(eng._lib.spf_blind_rotation_dev(eng._h, None, 1, 2, 0, p, None, p)), "null")
    assert eng.blind_rotation(shift[:0], glwe[:0]).shape == (0, P.glwe_len)     # B = 0: SPF_OK
    assert eng._lib.spf_blind_rotation_batch(eng._h, 0, 2, 0, None, None, None) == 0
