"""The host side of the GLWE keyswitch, automorphism and trace nodes of the gate graphs (`spf_graph_add_glwe_keyswitch`,
`spf_graph_add_glwe_automorphism`, `spf_graph_add_glwe_trace`): what needs no device.  A graph needs a context and a context needs
a device, so of the library's argument checks only the null handle can be reached here; the others are in
tests/test_gpu_glwe_keyswitch_graph.py.  `RecordedCircuit` records and refuses on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spf_amd
from spf_amd import FheOp, ValueKind, _ffi
from spf_amd.graph import GLWE_AUTOMORPHISM_NODE, GLWE_KEYSWITCH_NODE, GLWE_KSK_SLOTS, GLWE_TRACE_NODE

N = 2048
LOG_N = 11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("spf_graph_add_glwe_keyswitch", "spf_graph_add_glwe_automorphism", "spf_graph_add_glwe_trace")


def circuit():
    """(rec, glwe1 a, glwe1 b, lwe0, lwe1, ggsw1)"""
    rec = spf_amd.RecordedCircuit(N)
    a, b = rec.add_input(ValueKind.GLWE1, np.zeros(1)), rec.add_input(ValueKind.GLWE1, np.zeros(1))
    return (rec, a, b, rec.add_input(ValueKind.LWE0, np.zeros(1)), rec.add_input(ValueKind.LWE1, np.zeros(1)),
            rec.add_input(ValueKind.GGSW1, np.zeros(1)))


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_node_kinds_are_70_71_72_under_their_NODE_names_and_their_earlier_names():
    """the random differential tests of gate graphs draw every NODE_* name of spf_amd.graph; since their generator draws keyswitch
    keys the kinds are NODE_GLWE_KEYSWITCH / _AUTOMORPHISM / _TRACE, and the earlier names stay as aliases"""
    import spf_amd.graph as graph
    assert (GLWE_KEYSWITCH_NODE, GLWE_AUTOMORPHISM_NODE, GLWE_TRACE_NODE) == (70, 71, 72)
    assert (graph.NODE_GLWE_KEYSWITCH, graph.NODE_GLWE_AUTOMORPHISM, graph.NODE_GLWE_TRACE) == (70, 71, 72)
    names = {n: getattr(graph, n) for n in dir(graph) if n.startswith("NODE_")}
    assert names == {"NODE_UNPACK": 64, "NODE_PACK": 65, "NODE_ROT_CMUX": 66, "NODE_PUFKS": 67, "NODE_LWE_LINEAR": 68,
                     "NODE_GLWE_POLY_LINEAR": 69, "NODE_GLWE_KEYSWITCH": 70, "NODE_GLWE_AUTOMORPHISM": 71, "NODE_GLWE_TRACE": 72}
    assert GLWE_KSK_SLOTS == 16 and re.search(r"SPF_GLWE_KSK_SLOTS = 16\b", read("include", "spf_hip.h"))
    plan = read("spf_amd", "csrc", "spf_graph_plan.hpp")
    assert re.search(r"kNodeGlweKeyswitch = 70, kNodeGlweAutomorphism = 71, kNodeGlweTrace = 72\b", plan)


def test_the_header_the_rust_block_the_bindings_the_mirror_and_the_index_name_the_entry_points():
    header, rust, mirror, index = read("include", "spf_hip.h"), read("include", "spf_hip.rs"), read("include", "spf_evaluation.hpp"), read("INTEGRATION.md")
    assert "spf_status spf_graph_add_glwe_keyswitch(spf_graph *graph, uint32_t slot, uint32_t glwe_node, uint32_t *node_out);" in header
    assert "spf_status spf_graph_add_glwe_automorphism(spf_graph *graph, uint32_t round, uint32_t glwe_node, uint32_t *node_out);" in header
    assert "spf_status spf_graph_add_glwe_trace(spf_graph *graph, uint32_t glwe_node, uint32_t *node_out);" in header
    assert "pub fn spf_graph_add_glwe_keyswitch(graph: *mut spf_graph, slot: u32, glwe_node: u32, node_out: *mut u32) -> spf_status;" in rust
    assert "pub fn spf_graph_add_glwe_automorphism(graph: *mut spf_graph, round: u32, glwe_node: u32, node_out: *mut u32) -> spf_status;" in rust
    assert "pub fn spf_graph_add_glwe_trace(graph: *mut spf_graph, glwe_node: u32, node_out: *mut u32) -> spf_status;" in rust
    assert "Node glwe_keyswitch(uint32_t slot, Node glwe)" in mirror and "Node glwe_automorphism(uint32_t round, Node glwe)" in mirror
    assert "Node glwe_trace(Node glwe)" in mirror
    lib = _ffi.load_library()
    for name, n_args in zip(ENTRY_POINTS, (4, 4, 3)):
        assert f"`{name}` (:" in index, name
        assert len(getattr(lib, name).argtypes) == n_args, name
    # the header cites the reference function each constructor replaces
    doc = header[header.index("spf_graph_add_glwe_keyswitch     "):header.index("spf_status spf_graph_add_glwe_keyswitch(")]
    for cite in ("fft_ops.rs:457-495", "ops/polynomial/mod.rs:62-84", "ops/automorphisms/mod.rs:53-85"):
        assert cite in doc, cite
    for cls in (spf_amd.FheCircuit, spf_amd.RecordedCircuit):
        assert callable(cls.add_glwe_keyswitch) and callable(cls.add_glwe_automorphism) and callable(cls.add_glwe_trace)
    from spf_amd.mux_circuits import GraphBuilder
    assert callable(GraphBuilder.add_glwe_keyswitch) and callable(GraphBuilder.add_glwe_automorphism) and callable(GraphBuilder.add_glwe_trace)


def test_the_entry_points_refuse_a_null_handle_without_a_device():
    lib = _ffi.load_library()
    out = C.c_uint32(7)
    assert lib.spf_graph_add_glwe_keyswitch(None, 0, 0, C.byref(out)) == 1 and out.value == 7
    assert lib.spf_graph_add_glwe_automorphism(None, 1, 0, C.byref(out)) == 1 and out.value == 7
    assert lib.spf_graph_add_glwe_trace(None, 0, C.byref(out)) == 1 and out.value == 7


def levels(rec) -> list:
    lv = []
    for op, ins in zip(rec.op, rec.inputs):
        lv.append(0 if op < 0 else 1 + max(lv[i] for i in ins))
    return lv


def test_recorded_circuit_records_one_node_over_one_operand():
    rec, a, b, l0, l1, ggsw = circuit()
    x = rec.add_op(FheOp.GlweAdd, [a, b])                              # a GLWE one level up
    s = rec.add_glwe_keyswitch(15, x)                                  # the last slot
    r = rec.add_glwe_automorphism(LOG_N, s)                            # the last round, over another new node
    t = rec.add_glwe_trace(r)
    t0 = rec.add_glwe_trace(a)                                         # over an input
    assert [s, r, t, t0] == list(range(x + 1, x + 5))
    assert rec.op[s:] == [GLWE_KEYSWITCH_NODE, GLWE_AUTOMORPHISM_NODE, GLWE_TRACE_NODE, GLWE_TRACE_NODE]
    assert rec.kind[s:] == [int(ValueKind.GLWE1)] * 4 and rec.param[s:] == [15, LOG_N, 0, 0]
    assert rec.inputs[s:] == [(x,), (s,), (r,), (a,)]
    bits = rec.add_unpack(t, 3)                                        # the new nodes are ordinary GLWE nodes
    cm = rec.add_op(FheOp.CMux, [ggsw, t0, s])
    layer = rec.add_glwe_poly_linear(0, [cm, r], 2)
    k2 = rec.add_glwe_keyswitch(0, layer[1])
    lv = levels(rec)
    assert [lv[n] for n in (s, r, t, t0)] == [2, 3, 4, 1]              # one level above the operand
    assert [lv[n] for n in bits] == [5] * 3 and lv[cm] == 3 and [lv[n] for n in layer] == [4, 4] and lv[k2] == 5


def test_arrays_carry_the_nodes_and_round_trip():
    rec, a, b, l0, l1, _ = circuit()
    p = rec.add_pack([b, a])
    s = rec.add_glwe_keyswitch(4, p)
    r = rec.add_glwe_automorphism(2, a)
    t = rec.add_glwe_trace(s)
    rows = rec.add_glwe_poly_linear(9, [t, r], 2)
    rec.add_output(rows[1], ValueKind.GLWE1)
    rec.add_output(t, ValueKind.GLWE1)
    arr = rec.arrays()
    assert list(arr["op"][s:s + 3]) == [70, 71, 72] and list(arr["n_in"][s:s + 3]) == [1, 1, 1]
    assert list(arr["in"][s:s + 3, 0]) == [p, a, s] and list(arr["param"][s:s + 3]) == [4, 2, 0]
    assert list(arr["n_bits"][s:s + 3]) == [0, 0, 0] and list(arr["lin_rows"][s:s + 3]) == [0, 0, 0]
    assert list(arr["ext"]) == [b, a, t, r]                            # the new nodes have no operand list
    again = spf_amd.RecordedCircuit.from_arrays(arr, rec.kind, rec.host, N)
    assert again.op == rec.op and again.kind == rec.kind and again.param == rec.param and again.inputs == rec.inputs
    assert sorted(again.outputs) == sorted(rec.outputs)


def test_recorded_circuit_refuses_what_the_library_refuses():
    rec, a, b, l0, l1, ggsw = circuit()
    n_nodes = len(rec.op)
    ks, au, tr = rec.add_glwe_keyswitch, rec.add_glwe_automorphism, rec.add_glwe_trace
    for call, word in [(lambda: ks(GLWE_KSK_SLOTS, a), "slot must be in 0 .. 15"),
                       (lambda: ks(-1, a), "slot must be"),
                       (lambda: ks(None, a), "not an integer"),
                       (lambda: ks(True, a), "not an integer"),
                       (lambda: ks(1.0, a), "not an integer"),
                       (lambda: au(0, a), "round 0 outside 1 .. log2 N = 11"),
                       (lambda: au(LOG_N + 1, a), "round 12 outside 1 .. log2 N = 11"),
                       (lambda: au(None, a), "not an integer"),
                       (lambda: ks(0, l1), "not an L1 GLWE"),
                       (lambda: au(1, l0), "not an L1 GLWE"),
                       (lambda: tr(ggsw), "not an L1 GLWE"),
                       (lambda: tr(n_nodes), "not a node of this circuit"),
                       (lambda: ks(0, -1), "not a node of this circuit"),
                       (lambda: au(1, None), "not a node of this circuit"),
                       (lambda: tr(True), "not a node of this circuit")]:
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == 1 and word in str(e.value), (word, str(e.value))
        assert len(rec.op) == n_nodes                                   # nothing recorded
    small = spf_amd.RecordedCircuit(16)                                # the bound of the round is the recording's degree
    g = small.add_input(ValueKind.GLWE1, np.zeros(1))
    assert small.add_glwe_automorphism(4, g) == 1
    with pytest.raises(spf_amd.SpfError, match="round 5 outside 1 .. log2 N = 4"):
        small.add_glwe_automorphism(5, g)
    assert tr(a) == n_nodes                                             # ... and the recording still takes nodes


def test_the_per_operation_drivers_refuse_a_circuit_with_the_nodes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("driver_for_glwe_ks_test", os.path.join(ROOT, "tools", "driver.py"))
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    for add in (lambda rec, a: rec.add_glwe_keyswitch(0, a), lambda rec, a: rec.add_glwe_automorphism(1, a), lambda rec, a: rec.add_glwe_trace(a)):
        rec, a, *_ = circuit()
        driver._fhe_ops_only(rec)                                      # (a circuit of inputs alone passes)
        add(rec, a)
        with pytest.raises(RuntimeError, match="add_glwe_keyswitch / add_glwe_automorphism / add_glwe_trace"):
            driver._fhe_ops_only(rec)
