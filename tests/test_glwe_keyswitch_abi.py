"""The boundary of the GLWE keyswitch, the automorphism round and the trace without a GPU: the new names stand in the header, in
the Python binding, in the generated Rust block and in the integration guide; none of them ends in `_dev` (tests/stream_cases.py
holds a case for every `_dev` prototype); and a null context or group is refused, with a message, before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spf_amd
from spf_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["spf_load_glwe_keyswitch_key_std", "spf_glwe_keyswitch_slot_shape", "spf_glwe_keyswitch_batch", "spf_glwe_keyswitch_enqueue",
         "spf_glwe_automorphism_batch", "spf_glwe_automorphism_enqueue", "spf_glwe_trace_batch", "spf_glwe_trace_enqueue",
         "spf_last_glwe_keyswitch_kernel", "spf_group_load_glwe_keyswitch_key_std", "spf_group_glwe_keyswitch_batch",
         "spf_group_glwe_automorphism_batch", "spf_group_glwe_trace_batch"]


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


def test_no_prototype_of_the_section_ends_in_dev():
    hdr = read("include", "spf_hip.h")
    section = hdr[hdr.index("GLWE keyswitch, one automorphism round, homomorphic trace"):hdr.index("call coalescing: many threads")]
    protos = re.findall(r"\b(spf_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S))
    assert sorted(protos) == sorted(n for n in NAMES if not n.startswith("spf_group_")), protos
    assert not [p for p in protos if p.endswith("_dev")]


def test_the_slot_count_the_citations_and_the_bindings():
    hdr, rust = read("include", "spf_hip.h"), read("include", "spf_hip.rs")
    assert re.search(r"\bSPF_GLWE_KSK_SLOTS = 16\b", hdr)
    assert "pub const SPF_GLWE_KSK_SLOTS: spf_glwe_ksk_limits = 16;" in rust
    assert _ffi.GLWE_KSK_SLOTS == 16
    for cited in ("fft_ops.rs:457-495", "glwe_keyswitch.rs:26-55", "ops/polynomial/mod.rs:62-84", "ops/automorphisms/mod.rs:72-83",
                  "ops/automorphisms/mod.rs:53-85"):
        assert cited in hdr, cited
    assert '"glwe_keyswitch"' in hdr and "glwe_out == glwe_in" in hdr
    for method in ("load_glwe_keyswitch_key_std", "glwe_keyswitch", "glwe_automorphism", "glwe_trace", "glwe_keyswitch_enqueue",
                   "glwe_automorphism_enqueue", "glwe_trace_enqueue", "glwe_keyswitch_slot_shape", "last_glwe_keyswitch_kernel"):
        assert hasattr(spf_amd.Engine, method), method
    for method in ("keyswitch_glwe_to_glwe", "trace"):
        assert re.search(rf"def {method}\(", read("spf_amd", "evaluation.py")), method
        assert re.search(rf"void {method}\(", read("include", "spf_evaluation.hpp")), method


def test_a_null_context_and_null_pointers_are_refused_before_a_device_is_touched():
    lib = _ffi.load_library()
    x = np.zeros(64, dtype=np.uint64)
    p = x.ctypes.data_as(C.c_void_p)
    lg = C.c_uint32()
    for B in (0, 1, 1 << 40):
        for fn, lead in ((lib.spf_glwe_keyswitch_batch, (0,)), (lib.spf_glwe_automorphism_batch, (1,)), (lib.spf_glwe_trace_batch, ())):
            assert fn(None, *lead, B, p, p) == 1
            assert b"null" in lib.spf_last_error(None)
            assert fn(None, *lead, B, None, None) == 1
        for fn, lead in ((lib.spf_glwe_keyswitch_enqueue, (0,)), (lib.spf_glwe_automorphism_enqueue, (1,)), (lib.spf_glwe_trace_enqueue, ())):
            assert fn(None, None, *lead, B, p, p) == 1
        for fn, lead in ((lib.spf_group_glwe_keyswitch_batch, (0,)), (lib.spf_group_glwe_automorphism_batch, (1,)),
                         (lib.spf_group_glwe_trace_batch, ())):
            assert fn(None, *lead, B, p, p) == 1
            assert fn(None, *lead, B, None, None) == 1
    for slot in (0, 16):
        assert lib.spf_load_glwe_keyswitch_key_std(None, slot, p, 64, 7, 6) == 1
        assert b"null" in lib.spf_last_error(None)
        assert lib.spf_load_glwe_keyswitch_key_std(None, slot, None, 0, 7, 6) == 1
        assert lib.spf_group_load_glwe_keyswitch_key_std(None, slot, p, 64, 7, 6) == 1
        assert b"null group" in lib.spf_last_error(None)
    assert lib.spf_glwe_keyswitch_slot_shape(None, 0, C.byref(lg), C.byref(lg)) == 1
    assert lib.spf_glwe_keyswitch_slot_shape(None, 0, None, None) == 1
    assert lib.spf_last_glwe_keyswitch_kernel(None) == b""
    assert lib.spf_last_kernel_ms(None, b"glwe_keyswitch", None, None) == 1
