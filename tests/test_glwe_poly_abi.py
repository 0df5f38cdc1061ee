"""The boundary of the plaintext polynomial linear maps over GLWE ciphertexts without a GPU: the new names stand in the header,
in the Python binding, in the generated Rust block and in the integration guide, and a null context or group is refused, with a
message, before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spf_amd
from spf_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["spf_load_glwe_poly_weights", "spf_glwe_poly_linear_batch", "spf_glwe_poly_linear_enqueue", "spf_glwe_poly_slot_shape",
         "spf_last_glwe_poly_kernel", "spf_group_load_glwe_poly_weights", "spf_group_glwe_poly_linear_batch"]
LIMITS = {"SPF_GLWE_POLY_SLOTS": 64, "SPF_GLWE_POLY_MAX_ROWS": 4096, "SPF_GLWE_POLY_MAX_TERMS": 1 << 24}


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name", NAMES)
def test_the_name_stands_everywhere(name):
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "spf_hip.h"), flags=re.S)
    assert re.search(rf"\b{name}\s*\(", hdr), "include/spf_hip.h"
    assert name in {n for n, _, _ in _ffi.SYMBOLS}, "spf_amd/_ffi.py"
    assert re.search(rf"pub fn {name}\(", read("include", "spf_hip.rs")), "include/spf_hip.rs"
    assert f"`{name}`" in read("INTEGRATION.md"), "INTEGRATION.md"


def test_the_limits_and_the_section_of_the_header():
    hdr, rust = read("include", "spf_hip.h"), read("include", "spf_hip.rs")
    for const, value in LIMITS.items():
        assert re.search(rf"\b{const} = {value}\b", hdr), const
        assert f"pub const {const}: spf_glwe_poly_limits = {value};" in rust, const
    assert (_ffi.GLWE_POLY_SLOTS, _ffi.GLWE_POLY_MAX_ROWS, _ffi.GLWE_POLY_MAX_TERMS) == tuple(LIMITS.values())
    for cited in ("glwe_ciphertext_ops.rs:164-183", ":189-202", ":121-141", ":147-156", ":285-305", "math/polynomial.rs:114-197"):
        assert cited in hdr, cited
    assert '"glwe_poly_linear"' in hdr and "SPF_GLWE_POLY_PATH" in hdr
    for method in ("load_glwe_poly_weights", "glwe_poly_linear", "glwe_poly_slot_shape", "last_glwe_poly_kernel", "glwe_poly_linear_enqueue"):
        assert hasattr(spf_amd.Engine, method), method
    assert "load_glwe_poly_weights" in read("include", "spf_evaluation.hpp") and "glwe_poly_linear" in read("spf_amd", "evaluation.py")


def test_a_null_context_and_null_pointers_are_refused_before_a_device_is_touched():
    lib = _ffi.load_library()
    off = np.array([0, 1], dtype=np.uint32)
    exp = np.zeros(1, dtype=np.uint32)
    coef = np.ones(1, dtype=np.int64)
    x = np.zeros(64, dtype=np.uint64)
    o, e, c, p = (a.ctypes.data_as(C.c_void_p) for a in (off, exp, coef, x))
    sz, flag = C.c_size_t(), C.c_int()
    for B in (0, 1, 1 << 40):
        assert lib.spf_glwe_poly_linear_batch(None, 0, B, p, p) == 1
        assert b"null" in lib.spf_last_error(None)
        assert lib.spf_glwe_poly_linear_enqueue(None, None, 0, B, p, p) == 1
        assert lib.spf_glwe_poly_linear_batch(None, 0, B, None, None) == 1
        assert lib.spf_group_glwe_poly_linear_batch(None, 0, B, p, p) == 1
        assert lib.spf_group_glwe_poly_linear_batch(None, 0, B, None, None) == 1
    for slot in (0, 64):
        assert lib.spf_load_glwe_poly_weights(None, slot, 1, 1, o, e, c, None) == 1
        assert b"null context" in lib.spf_last_error(None)
        assert lib.spf_load_glwe_poly_weights(None, slot, 1, 1, None, None, None, None) == 1
        assert lib.spf_group_load_glwe_poly_weights(None, slot, 1, 1, o, e, c, None) == 1
        assert b"null group" in lib.spf_last_error(None)
    assert lib.spf_glwe_poly_slot_shape(None, 0, C.byref(sz), C.byref(sz), C.byref(sz), C.byref(flag)) == 1
    assert lib.spf_glwe_poly_slot_shape(None, 0, None, None, None, None) == 1
    assert lib.spf_last_glwe_poly_kernel(None) == b""
    assert lib.spf_last_kernel_ms(None, b"glwe_poly_linear", None, None) == 1
