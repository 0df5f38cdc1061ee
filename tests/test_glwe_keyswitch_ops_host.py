"""The GLWE keyswitch, one automorphism round and the homomorphic trace as operations of the table (spf_amd/csrc/spf_ops.hpp), behind
the generic doors (`spf_graph_add_op`, `spf_pool_submit_op_v`) and as submits of the pool: what needs no device.

tests/cpp/glwe_keyswitch_ops.cpp is a stand-alone program over the two HIP-free headers, built with the system g++ under
AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into python): the three rows,
`pool_op_of` both ways, `shape()`, `op_param` at N = 16 and N = 2048, and the plan of a graph through the generic door equal field by
field to the plan through the named constructors' nodes.  The Python part: the enum values equal the header's, the six submits are
exported with the binding's signatures, null handles are refused, and `RecordedCircuit.add_op` records the named constructors'
nodes.  The GPU side is tests/test_gpu_glwe_keyswitch_pool.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import spf_amd
from spf_amd import FheOp, KeyswitchOp, TableOp, ValueKind, _ffi
from spf_amd.graph import GLWE_AUTOMORPHISM_NODE, GLWE_KEYSWITCH_NODE, GLWE_TRACE_NODE, graph_op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, P, PP, PT = C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)
SUBMITS = {"spf_pool_submit_glwe_keyswitch": [P, U32, P, P, PT], "spf_pool_submit_glwe_automorphism": [P, U32, P, P, PT],
           "spf_pool_submit_glwe_trace": [P, P, P, PT], "spf_pool_submit_glwe_keyswitch_v": [P, U32, P, PP, PT],
           "spf_pool_submit_glwe_automorphism_v": [P, U32, P, PP, PT], "spf_pool_submit_glwe_trace_v": [P, P, PP, PT]}
INVALID = 1


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glwe_keyswitch_ops") / "glwe_keyswitch_ops")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "glwe_keyswitch_ops.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_every_check_of_the_program_passes_without_a_sanitizer_report(output):
    assert "FAILED" not in output and output.rstrip().endswith("glwe_keyswitch_ops ok"), output[-3000:]
    assert "rows ok" in output.splitlines() and "parameters ok" in output.splitlines()


@pytest.mark.parametrize("mode", ["keyswitch", "automorphism", "trace"])
@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_the_generic_door_plans_as_the_named_constructors(output, mode, B):
    for glwe in (256, 128, 32768):      # consecutive inputs, inputs padded apart, the tuned context's GLWE
        assert f"scattered {mode} B={B} glwe={glwe}: 2 groups of the three kinds ok" in output.splitlines(), output[-3000:]
    assert "chain glwe=256: 6 groups of the three kinds ok" in output.splitlines()
    assert "chain glwe=128: 6 groups of the three kinds ok" in output.splitlines()


def test_the_enum_values_are_the_headers():
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "spf_hip.h"), flags=re.S)
    values = {name: int(v) for name, v in re.findall(r"\b(SPF_OP_\w+)\s*=\s*(\d+)", hdr)}
    assert values["SPF_OP_GLWE_KEYSWITCH"] == 12 and values["SPF_OP_GLWE_AUTOMORPHISM"] == 13 and values["SPF_OP_GLWE_TRACE"] == 14
    assert len(values) == 15 and sorted(values.values()) == list(range(15))
    assert (int(FheOp.GLWE_KEYSWITCH), int(FheOp.GLWE_AUTOMORPHISM), int(FheOp.GLWE_TRACE)) == (12, 13, 14)
    assert FheOp.GLWE_KEYSWITCH is KeyswitchOp.GLWE_KEYSWITCH and graph_op(13) is KeyswitchOp.GLWE_AUTOMORPHISM and graph_op(14) is FheOp.GLWE_TRACE
    assert graph_op(11) is TableOp.PBS_BIVARIATE and graph_op(9) is FheOp.MulXN           # the existing twelve as they were
    assert len(list(FheOp)) == 10 and len(list(TableOp)) == 2 and len(list(KeyswitchOp)) == 3
    for name, value in values.items():                                                      # ... in the generated Rust block too
        assert f"pub const {name}: spf_graph_op = {value};" in read("include", "spf_hip.rs"), name
    ops = read("spf_amd", "csrc", "spf_ops.hpp")
    assert re.search(r"OP_GLWE_KEYSWITCH = 14, OP_GLWE_AUTOMORPHISM = 15, OP_GLWE_TRACE = 16,\s*N_OPS = 17", ops)
    assert "hip/hip_runtime.h" not in ops and "hipStream_t" not in ops                     # the header stays free of HIP


@pytest.mark.parametrize("name", sorted(SUBMITS))
def test_the_submit_is_exported_with_the_bindings_signature(name):
    sig = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    assert sig[name] == (C.c_int, SUBMITS[name]), sig.get(name)
    lib = _ffi.load_library()
    assert getattr(lib, name).argtypes == SUBMITS[name] and getattr(lib, name).restype is C.c_int
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "spf_hip.h"), flags=re.S)
    assert re.search(rf"\bspf_status {name}\s*\(spf_pool \*pool,", hdr), "include/spf_hip.h"
    assert re.search(rf"pub fn {name}\(", read("include", "spf_hip.rs")), "include/spf_hip.rs"
    assert f"`{name}`" in read("INTEGRATION.md"), "INTEGRATION.md"


def test_the_mirrors_have_the_methods():
    for method in ("glwe_keyswitch", "glwe_automorphism", "glwe_trace", "glwe_keyswitch_v", "glwe_automorphism_v", "glwe_trace_v"):
        assert callable(getattr(spf_amd.Pool, method)), method
    hpp = read("include", "spf_evaluation.hpp")
    pooled = hpp[hpp.index("class PooledEvaluation"):]
    for method, op in (("keyswitch_glwe_to_glwe", "SPF_OP_GLWE_KEYSWITCH"), ("glwe_automorphism", "SPF_OP_GLWE_AUTOMORPHISM"), ("trace", "SPF_OP_GLWE_TRACE")):
        assert re.search(rf"void {method}\(L1GlweCiphertext& output, const L1GlweCiphertext& input", pooled) and op in pooled, method
    assert re.search(r"def glwe_automorphism\(", read("spf_amd", "evaluation.py"))


def test_entry_points_refuse_null_handles_without_a_device():
    lib = _ffi.load_library()
    x = np.zeros(64, dtype=np.uint64)
    p = x.ctypes.data_as(C.c_void_p)
    for op in (12, 13, 14):
        vals = (C.c_void_p * 1)()
        h, t = C.c_void_p(), C.c_uint64(77)
        assert lib.spf_pool_submit_op_v(None, op, vals, 1, 1, C.byref(h), C.byref(t)) == INVALID and not h.value and t.value == 77
        node = C.c_uint32(7)
        assert lib.spf_graph_add_op(None, op, (C.c_uint32 * 1)(0), 1, 1, C.byref(node)) == INVALID and node.value == 7
    for lead in ((0,), (16,)):
        for fn in (lib.spf_pool_submit_glwe_keyswitch, lib.spf_pool_submit_glwe_automorphism):
            t = C.c_uint64(77)
            assert fn(None, *lead, p, p, C.byref(t)) == INVALID and t.value == 77
        for fn in (lib.spf_pool_submit_glwe_keyswitch_v, lib.spf_pool_submit_glwe_automorphism_v):
            h, t = C.c_void_p(), C.c_uint64(77)
            assert fn(None, *lead, None, C.byref(h), C.byref(t)) == INVALID and not h.value and t.value == 77
    h, t = C.c_void_p(), C.c_uint64(77)
    assert lib.spf_pool_submit_glwe_trace(None, p, p, C.byref(t)) == INVALID and t.value == 77
    assert lib.spf_pool_submit_glwe_trace_v(None, None, C.byref(h), C.byref(t)) == INVALID and not h.value and t.value == 77


def test_recorded_circuit_records_the_named_constructors_nodes_through_add_op():
    rec = spf_amd.RecordedCircuit(16)
    a = rec.add_input(ValueKind.GLWE1, np.zeros(1))
    l1 = rec.add_input(ValueKind.LWE1, np.zeros(1))
    k = rec.add_op(FheOp.GLWE_KEYSWITCH, [a], 15)
    r = rec.add_op(FheOp.GLWE_AUTOMORPHISM, [k], 4)
    t = rec.add_op(FheOp.GLWE_TRACE, [r], 99)                  # the trace's parameter is forced to 0
    named = spf_amd.RecordedCircuit(16)
    named.add_input(ValueKind.GLWE1, np.zeros(1))
    named.add_input(ValueKind.LWE1, np.zeros(1))
    named.add_glwe_trace(named.add_glwe_automorphism(4, named.add_glwe_keyswitch(15, a)))
    assert rec.op[k:] == [GLWE_KEYSWITCH_NODE, GLWE_AUTOMORPHISM_NODE, GLWE_TRACE_NODE] == named.op[k:]
    assert rec.param == named.param and rec.param[k:] == [15, 4, 0] and rec.inputs == named.inputs and rec.kind == named.kind
    n_nodes = len(rec.op)
    for call, word in [(lambda: rec.add_op(FheOp.GLWE_KEYSWITCH, [a], 16), "slot must be in 0 .. 15"),
                       (lambda: rec.add_op(FheOp.GLWE_AUTOMORPHISM, [a], 0), "round 0 outside 1 .. log2 N = 4"),
                       (lambda: rec.add_op(FheOp.GLWE_AUTOMORPHISM, [a], 5), "round 5 outside 1 .. log2 N = 4"),
                       (lambda: rec.add_op(FheOp.GLWE_TRACE, [a, a]), "unknown operation: value 14 over 2 operands"),
                       (lambda: rec.add_op(FheOp.GLWE_KEYSWITCH, [], 0), "unknown operation: value 12 over 0 operands"),
                       (lambda: rec.add_op(FheOp.GLWE_TRACE, [l1]), "not an L1 GLWE"),
                       (lambda: rec.add_op(FheOp.GLWE_TRACE, [n_nodes]), "not a node")]:
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == 1 and word in str(e.value), (word, str(e.value))
        assert len(rec.op) == n_nodes and t == n_nodes - 1
