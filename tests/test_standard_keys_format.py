"""`ComputeKeyNonFft` (crypto/keys.rs:145-159), the reference's portable key form: its bincode layout in spf_amd.keys — round trip,
exact bytes, and every rejection — and the argument checks of the C entry points that take keys and polynomials in standard
(integer) form, which must answer before they touch a device.  No GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

import spf_amd
from spf_amd import _ffi
from spf_amd.keys import (ComputeKeyNonFft, KeyFormatError, parse_compute_key, parse_compute_key_nonfft, serialize_compute_key,
                          serialize_compute_key_nonfft)

P = spf_amd.DEFAULT_128.replace(lwe_dimension=2)
FIELDS = ("bs_key", "ks_key", "auto_key", "ss_key")     # keys.rs:145-159 — not ComputeKey's order
COUNTS = (2 * P.bsk_complex, P.ksk_words, 2 * P.ak_complex, 2 * P.ssk_complex)


def _ck(seed=0) -> ComputeKeyNonFft:
    r = np.random.default_rng(seed)
    return ComputeKeyNonFft(*[r.integers(0, 1 << 64, n, dtype=np.uint64) for n in COUNTS])


def _offsets():
    """byte offset of each field's count"""
    out, off = [], 0
    for n in COUNTS:
        out.append(off)
        off += 8 + 8 * n
    return out, off


def test_counts_are_the_polynomial_words_of_the_fft_layouts():
    D = spf_amd.DEFAULT_128
    assert 2 * D.bsk_complex == 637 * 2 * 2 * 2 * 2048 and 2 * D.ak_complex == 11 * 6 * 2 * 2048 and 2 * D.ssk_complex == 15 * 2 * 2048
    assert 2 * D.bsk_complex * 8 == D.bsk_complex * 16 == 83_492_864        # a polynomial and its spectrum: the same bytes


def test_roundtrip_and_layout():
    ck = _ck()
    buf = serialize_compute_key_nonfft(ck)
    offs, total = _offsets()
    assert len(buf) == total == 4 * 8 + 8 * sum(COUNTS)
    for name, n, off in zip(FIELDS, COUNTS, offs):      # u64 LE count, then the words little-endian, fields in declaration order
        assert struct.unpack_from("<Q", buf, off)[0] == n, name
        assert struct.unpack_from("<Q", buf, off + 8)[0] == int(getattr(ck, name)[0]), name
        assert struct.unpack_from("<Q", buf, off + 8 * n)[0] == int(getattr(ck, name)[-1]), name
    back = parse_compute_key_nonfft(buf + b"trailing bytes are allowed", P)
    for name in FIELDS:
        got = getattr(back, name)
        assert got.dtype == np.uint64 and np.array_equal(got, getattr(ck, name)), name
    assert serialize_compute_key_nonfft(back) == buf


def test_every_field_rejects_a_wrong_count_and_a_truncation():
    buf = serialize_compute_key_nonfft(_ck(1))
    offs, total = _offsets()
    for name, n, off in zip(FIELDS, COUNTS, offs):
        for wrong in (n + 1, n - 1, 0, n // 2, (1 << 64) - 1):
            bad = bytearray(buf)
            bad[off:off + 8] = struct.pack("<Q", wrong)
            with pytest.raises(KeyFormatError, match=name):
                parse_compute_key_nonfft(bytes(bad), P)
        for cut in (off, off + 3, off + 7):                       # before / inside the count
            with pytest.raises(KeyFormatError, match=name):
                parse_compute_key_nonfft(buf[:cut], P)
        for cut in (off + 8, off + 8 + 8 * (n // 2) + 5, off + 8 + 8 * n - 1):   # inside the words
            with pytest.raises(KeyFormatError, match=name):
                parse_compute_key_nonfft(buf[:cut], P)
    with pytest.raises(KeyFormatError):
        parse_compute_key_nonfft(b"", P)
    with pytest.raises(KeyFormatError):
        parse_compute_key_nonfft(buf, spf_amd.DEFAULT_128)        # another parameter set
    with pytest.raises(KeyFormatError):   # the reference's malformed-length vector (safe_bincode.rs:98-117)
        parse_compute_key_nonfft(bytes([253, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x1, 0x2, 0x3, 0x4]), P)


def test_the_two_key_forms_are_not_taken_for_each_other():
    r = np.random.default_rng(2)
    c = lambda n: r.standard_normal(n) + 1j * r.standard_normal(n)   # noqa: E731
    fft_blob = serialize_compute_key(spf_amd.ComputeKey(bs_key=c(P.bsk_complex), ks_key=r.integers(0, 1 << 64, P.ksk_words, dtype=np.uint64),
                                                        ss_key=c(P.ssk_complex), auto_key=c(P.ak_complex)))
    with pytest.raises(KeyFormatError, match="bs_key"):             # counts complex numbers, ss_key before auto_key
        parse_compute_key_nonfft(fft_blob, P)
    std_blob = serialize_compute_key_nonfft(_ck(3))
    with pytest.raises(KeyFormatError):
        parse_compute_key(std_blob, P)
    # the same words with the last two fields in ComputeKey's order: auto_key's count is then ss_key's
    ck = _ck(3)
    swapped = serialize_compute_key_nonfft(ComputeKeyNonFft(ck.bs_key, ck.ks_key, ck.ss_key, ck.auto_key))
    with pytest.raises(KeyFormatError, match="auto_key"):
        parse_compute_key_nonfft(swapped, P)


def test_serializer_refuses_anything_but_integer_words():
    ck = _ck(4)
    ck.auto_key = ck.auto_key.astype(np.float64)
    with pytest.raises(KeyFormatError, match="auto_key"):
        serialize_compute_key_nonfft(ck)


@pytest.fixture(scope="module")
def lib():
    spf_amd.build_library()
    return spf_amd.load_library()


def test_c_entry_points_refuse_null_arguments_without_a_device(lib):
    """SPF_ERR_INVALID_ARGUMENT (1) before any HIP call: this runs where no GPU exists.  (Wrong lengths on a context are refused
    before the device as well: tools/fuzz_host.cpp holds that table for a context made by hand, tests/test_asan_host.py runs it,
    and tests/test_gpu_standard_keys.py repeats it on a real one.)"""
    words = np.zeros(16, dtype=np.uint64)
    spec = np.zeros(16, dtype=np.float64)
    blob = np.zeros(64, dtype=np.uint8)
    w, s, b = _ffi._ptr(words), _ffi._ptr(spec), _ffi._ptr(blob)
    assert lib.spf_poly_fft_dev(None, None, 1, w, s) == 1
    assert lib.spf_poly_fft_batch(None, 1, w, s) == 1
    for name in ("bootstrap", "automorphism", "scheme_switch"):
        assert getattr(lib, f"spf_load_{name}_key_std")(None, w, 16) == 1, name
        assert getattr(lib, f"spf_group_load_{name}_key_std")(None, w, 16) == 1, name
    assert lib.spf_load_compute_key_nonfft_bincode(None, b, 64) == 1
    assert lib.spf_group_load_compute_key_nonfft_bincode(None, b, 64) == 1
    assert b"null" in lib.spf_last_error(None)


def test_python_methods_validate_their_operands_before_the_library_is_called():
    """an Engine cannot exist here; the checks are plain functions of (params, operand)"""
    eng = object.__new__(spf_amd.Engine)
    eng.params = P
    with pytest.raises(spf_amd.SpfError, match="uint64"):
        eng._std_words("load_bootstrap_key_std", np.zeros(2 * P.bsk_complex, dtype=np.complex128), P.bsk_complex)
    with pytest.raises(spf_amd.SpfError, match="expected"):
        eng._std_words("load_bootstrap_key_std", np.zeros(P.bsk_complex, dtype=np.uint64), P.bsk_complex)   # counted in complex
    assert eng._std_words("load_scheme_switch_key_std", np.zeros((15, 2, 2048), dtype=np.uint64), P.ssk_complex).shape == (15 * 2 * 2048,)
    for bad in (np.zeros((3, 1024), dtype=np.uint64), np.zeros((3, 2048), dtype=np.int64), [0] * 2048, np.uint64(3)):
        with pytest.raises(spf_amd.SpfError, match="poly_fft"):
            eng.poly_fft(bad)
    grp = object.__new__(spf_amd.Group)
    grp.params = P
    grp._lib = _ffi._GroupLib(spf_amd.load_library())
    with pytest.raises(spf_amd.SpfError, match="no group form"):       # the primitive belongs to a member
        grp.poly_fft(np.zeros((1, 2048), dtype=np.uint64))
    # ... and the loaders resolve to their group forms
    assert grp._lib.spf_load_bootstrap_key_std.__name__ == "spf_group_load_bootstrap_key_std"
    assert grp._lib.spf_load_compute_key_nonfft_bincode.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t]
