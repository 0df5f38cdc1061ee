"""The boundary of ring packing without a GPU: the new names stand in the header, in the Python binding, in the generated Rust
block and in the integration guide; none of them ends in `_dev` (tests/stream_cases.py holds a case for every `_dev` prototype);
the header states the strided layout; and a null context or group is refused, with a message, before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spf_amd
from spf_amd import _ffi, packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["spf_lwe_ring_pack_batch", "spf_lwe_ring_pack_scratch_words", "spf_lwe_ring_pack_enqueue", "spf_last_lwe_ring_pack_kernel",
         "spf_group_lwe_ring_pack_batch"]


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
    assert not name.endswith("_dev")


def test_the_header_states_the_operation_the_layout_and_the_family():
    hdr = read("include", "spf_hip.h")
    section = hdr[hdr.index("ring packing: LWE or GLWE ciphertexts into one GLWE"):hdr.index("measurement hooks (bench.py)")]
    protos = re.findall(r"\b(spf_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S))
    assert sorted(protos) == sorted(n for n in NAMES if not n.startswith("spf_group_")), protos
    for said in ("STRIDED", "j * N / p", "log_stride = log2(N / p)", "spf_sample_extract_l1_each_", "spf_glwe_poly_linear_",
                 "glwe_ciphertext_ops.rs:31-76", "ops/automorphisms/mod.rs:53-85", "SPF_LWE_RING_PACK_SCRATCH_BYTES", "m + 1"):
        assert said in section, said
    assert '"lwe_ring_pack"' in hdr[hdr.index("measurement hooks (bench.py)"):]


def test_the_bindings_and_the_strided_helpers():
    for method in ("lwe_ring_pack", "lwe_ring_pack_enqueue", "lwe_ring_pack_scratch_words", "last_lwe_ring_pack_kernel"):
        assert hasattr(spf_amd.Engine, method), method
    assert re.search(r"def lwe_ring_pack\(", read("spf_amd", "evaluation.py"))
    assert re.search(r"void lwe_ring_pack\(", read("include", "spf_evaluation.hpp"))
    P = spf_amd.DEFAULT_128
    assert list(packed.strided_positions(4, P)) == [0, 512, 1024, 1536]
    assert list(packed.strided_positions(1, P)) == [0] and len(packed.strided_positions(2048, P)) == 2048
    for bad in (0, 3, 4096):
        with pytest.raises(ValueError):
            packed.strided_positions(bad, P)
    poly = packed.strided_plaintext([5, 6, 7, (1 << 64) + 9], P)
    assert poly.dtype == np.uint64 and np.count_nonzero(poly) == 4
    assert list(packed.strided_decode(poly, 4, P)) == [5, 6, 7, 9]


def test_a_null_context_is_refused_before_a_device_is_touched():
    lib = _ffi.load_library()
    x = np.zeros(64, dtype=np.uint64)
    p = x.ctypes.data_as(C.c_void_p)
    w = C.c_size_t()
    for B in (0, 1, 1 << 40):
        assert lib.spf_lwe_ring_pack_batch(None, 1, 4, B, p, p) == 1
        assert b"null" in lib.spf_last_error(None)
        assert lib.spf_lwe_ring_pack_batch(None, 1, 4, B, None, None) == 1
        assert lib.spf_lwe_ring_pack_enqueue(None, None, 1, 4, B, p, p, 64, p) == 1
        assert lib.spf_group_lwe_ring_pack_batch(None, 1, 4, B, p, p) == 1
        assert lib.spf_lwe_ring_pack_scratch_words(None, 4, B, C.byref(w)) == 1
    assert lib.spf_last_lwe_ring_pack_kernel(None) == b""
    assert lib.spf_last_kernel_ms(None, b"lwe_ring_pack", None, None) == 1
