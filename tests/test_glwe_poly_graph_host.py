"""The host side of the plaintext polynomial linear maps over GLWE ciphertexts as gate-graph nodes
(`spf_graph_add_glwe_poly_linear`): what needs no device.  A graph needs a context and a context needs a device, so of the
library's argument checks only the null handle can be reached here; the others are in tests/test_gpu_glwe_poly_linear_graph.py.
`RecordedCircuit` records and refuses on the host, and the last test is the condition of the GPU suite's decrypt-level case: on
the ORACLE alone — encrypt, `poly_linear_ref`, sample extract, decrypt — the layer gives the bits of (a << s) ^ b."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind, _ffi
from spf_amd.graph import GLWE_POLY_LINEAR_NODE, NODE_LWE_LINEAR
from tests import glwe_poly_cases as GC
from tests import glwe_poly_graph_cases as G

N = 2048
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def circuit():
    """(rec, glwe1 a, glwe1 b, lwe0, lwe1, ggsw1)"""
    rec = spf_amd.RecordedCircuit(N)
    a, b = rec.add_input(ValueKind.GLWE1, np.zeros(1)), rec.add_input(ValueKind.GLWE1, np.zeros(1))
    return (rec, a, b, rec.add_input(ValueKind.LWE0, np.zeros(1)), rec.add_input(ValueKind.LWE1, np.zeros(1)),
            rec.add_input(ValueKind.GGSW1, np.zeros(1)))


def test_the_node_kind_is_69_under_its_NODE_name_and_its_earlier_name():
    """the random differential tests of gate graphs draw every NODE_* name of spf_amd.graph (tests/test_graph_fuzz_host.py); since
    their generator draws polynomial weights the kind is NODE_GLWE_POLY_LINEAR, and GLWE_POLY_LINEAR_NODE stays as its alias"""
    import spf_amd.graph as graph
    assert GLWE_POLY_LINEAR_NODE == graph.NODE_GLWE_POLY_LINEAR == 69
    names = {n: getattr(graph, n) for n in dir(graph) if n.startswith("NODE_")}
    assert names == {"NODE_UNPACK": 64, "NODE_PACK": 65, "NODE_ROT_CMUX": 66, "NODE_PUFKS": 67, "NODE_LWE_LINEAR": 68,
                     "NODE_GLWE_POLY_LINEAR": 69, "NODE_GLWE_KEYSWITCH": 70, "NODE_GLWE_AUTOMORPHISM": 71, "NODE_GLWE_TRACE": 72}
    assert graph.GLWE_POLY_SLOTS == G.SLOTS == _ffi.GLWE_POLY_SLOTS and graph.GLWE_POLY_MAX_ROWS == G.MAX_ROWS == _ffi.GLWE_POLY_MAX_ROWS


def test_the_header_the_rust_block_the_bindings_and_the_index_name_the_entry_point():
    with open(os.path.join(ROOT, "include", "spf_hip.h")) as f:
        header = f.read()
    assert re.search(r"spf_status spf_graph_add_glwe_poly_linear\(spf_graph \*graph, uint32_t slot, const uint32_t \*glwe_nodes", header)
    assert re.search(r"SPF_GLWE_POLY_MAX_ROWS = %d\b" % G.MAX_ROWS, header) and re.search(r"SPF_GLWE_POLY_SLOTS = %d\b" % G.SLOTS, header)
    with open(os.path.join(ROOT, "include", "spf_hip.rs")) as f:
        assert ("pub fn spf_graph_add_glwe_poly_linear(graph: *mut spf_graph, slot: u32, glwe_nodes: *const u32, K: usize, M: usize, "
                "nodes_out: *mut u32) -> spf_status;") in f.read()
    with open(os.path.join(ROOT, "include", "spf_evaluation.hpp")) as f:
        assert "std::vector<Node> glwe_poly_linear(uint32_t slot, const std::vector<Node>& glwes, size_t M)" in f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "`spf_graph_add_glwe_poly_linear` (:" in f.read()
    lib = _ffi.load_library()
    assert lib.spf_graph_add_glwe_poly_linear.argtypes is not None and len(lib.spf_graph_add_glwe_poly_linear.argtypes) == 6
    assert callable(spf_amd.FheCircuit.add_glwe_poly_linear) and callable(spf_amd.RecordedCircuit.add_glwe_poly_linear)


def test_the_entry_point_refuses_a_null_handle_without_a_device():
    lib = _ffi.load_library()
    nodes = (C.c_uint32 * 3)(0, 1, 2)
    out = (C.c_uint32 * 2)(7, 7)
    assert lib.spf_graph_add_glwe_poly_linear(None, 0, nodes, 3, 2, out) == 1 and list(out) == [7, 7]


def levels(rec) -> list:
    lv = []
    for op, ins in zip(rec.op, rec.inputs):
        lv.append(0 if op < 0 else 1 + max(lv[i] for i in ins))
    return lv


def test_recorded_circuit_records_a_layer_as_m_nodes_over_one_operand_list():
    rec, a, b, l0, l1, ggsw = circuit()
    x = rec.add_op(FheOp.GlweAdd, [a, b])                              # a GLWE one level up
    rows = rec.add_glwe_poly_linear(5, [a, x, a], 4)                   # GLWE nodes of any origin; repeats allowed
    assert rows == list(range(x + 1, x + 5))
    assert rec.op[rows[0]:] == [GLWE_POLY_LINEAR_NODE] * 4 and rec.kind[rows[0]:] == [int(ValueKind.GLWE1)] * 4
    assert rec.param[rows[0]:] == [0, 1, 2, 3] and rec.inputs[rows[0]:] == [(a, x, a)] * 4
    assert rec.linear_of(rows[2]) == (5, 4)
    low = rec.add_glwe_poly_linear(63, [b], 1)                         # one operand, one row, the last slot
    bits = rec.add_unpack(rows[3], 3)                                  # the new nodes are ordinary GLWE nodes
    cm = rec.add_op(FheOp.CMux, [ggsw, rows[0], low[0]])
    again = rec.add_glwe_poly_linear(0, [cm, rows[1], low[0]], 2)
    assert len(rec.add_glwe_poly_linear(0, [a], G.MAX_ROWS)) == G.MAX_ROWS   # M at the limit is accepted
    lv = levels(rec)
    assert [lv[n] for n in rows] == [2] * 4                            # one level above the highest operand (the XOR: 1)
    assert [lv[n] for n in low] == [1] and [lv[n] for n in bits] == [3] * 3 and [lv[n] for n in again] == [4, 4]


def test_arrays_carry_the_layer_and_round_trip_next_to_an_lwe_layer():
    rec, a, b, l0, l1, _ = circuit()
    p = rec.add_pack([b, a])
    rows = rec.add_glwe_poly_linear(9, [b, a, b], 2)
    lwe = rec.add_lwe_linear(7, [l1, l1], 2)                           # the LWE layer shares lin_slot / lin_rows and the ext list
    more = rec.add_glwe_poly_linear(10, rows, 3)
    k = rec.add_pack([p, more[1]])
    rec.add_output(more[2], ValueKind.GLWE1)
    rec.add_output(rows[0], ValueKind.GLWE1)
    arr = rec.arrays()
    at = rows[0]
    assert list(arr["op"][at:at + 7]) == [GLWE_POLY_LINEAR_NODE] * 2 + [NODE_LWE_LINEAR] * 2 + [GLWE_POLY_LINEAR_NODE] * 3
    assert list(arr["n_in"][at:at + 7]) == [0] * 7
    assert list(arr["n_bits"][at:at + 7]) == [3, 3, 2, 2, 2, 2, 2] and list(arr["param"][at:at + 7]) == [0, 1, 0, 1, 0, 1, 2]
    assert list(arr["lin_slot"][at:at + 7]) == [9, 9, 7, 7, 10, 10, 10] and list(arr["lin_rows"][at:at + 7]) == [2, 2, 2, 2, 3, 3, 3]
    # the operand lists in node order, ONE per call: [pack | layer 9 | LWE layer 7 | layer 10 | pack]
    assert list(arr["ext"]) == [b, a, b, a, b, l1, l1, rows[0], rows[1], p, more[1]]
    assert list(arr["ext_at"][[p, rows[0], rows[1], lwe[0], lwe[1], more[0], more[2], k]]) == [0, 2, 2, 5, 5, 7, 7, 9]
    assert arr["lin_rows"][p] == 0 and arr["lin_rows"][k] == 0 and list(np.flatnonzero(arr["keep"])) == [rows[0], more[2]]
    again = spf_amd.RecordedCircuit.from_arrays(arr, rec.kind, rec.host, N)
    assert again.op == rec.op and again.kind == rec.kind and again.param == rec.param and again.inputs == rec.inputs
    assert again._linear == rec._linear and sorted(again.outputs) == sorted(rec.outputs)


def test_recorded_circuit_refuses_what_the_library_refuses():
    rec, a, b, l0, l1, ggsw = circuit()
    n_nodes = len(rec.op)
    lin = rec.add_glwe_poly_linear
    for call, word in [(lambda: lin(G.SLOTS, [a], 1), "slot"),
                       (lambda: lin(-1, [a], 1), "slot"),
                       (lambda: lin(None, [a], 1), "slot"),
                       (lambda: lin(True, [a], 1), "slot"),
                       (lambda: lin(0, [], 1), "K = 0"),
                       (lambda: lin(0, [a], 0), "M must be"),
                       (lambda: lin(0, [a], G.MAX_ROWS + 1), "M must be"),
                       (lambda: lin(0, [a], None), "M must be"),
                       (lambda: lin(0, [a], 1.0), "M must be"),
                       (lambda: lin(0, [l1], 1), "not an L1 GLWE"),
                       (lambda: lin(0, [a, l0], 1), "not an L1 GLWE"),
                       (lambda: lin(0, [a, ggsw], 1), "not an L1 GLWE"),
                       (lambda: lin(0, [a, n_nodes], 1), "not a node"),
                       (lambda: lin(0, [-1], 1), "not a node"),
                       (lambda: lin(0, [None], 1), "not a node")]:
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == 1 and "add_glwe_poly_linear" in str(e.value) and word in str(e.value), str(e.value)
        assert len(rec.op) == n_nodes                                          # nothing recorded
    assert lin(0, [a, b], 2) == [n_nodes, n_nodes + 1]


def test_the_builder_of_mux_circuits_passes_the_layer_on():
    from spf_amd.mux_circuits import GraphBuilder
    rec, a, b, _, _, _ = circuit()
    rows = GraphBuilder(rec).add_glwe_poly_linear(3, [a, b], 2)
    assert rec.op[rows[0]:] == [GLWE_POLY_LINEAR_NODE] * 2 and rec._linear[rows[1]] == (3, 2)


def test_native_per_operation_drivers_say_that_they_cannot_walk_the_node():
    """pushing a recording by handle refuses the node with the message the LWE layer gets"""
    from tools import driver
    rec = spf_amd.RecordedCircuit(N)
    rec.add_glwe_poly_linear(0, [rec.add_input(ValueKind.GLWE1, np.zeros(1))], 1)
    lwe = spf_amd.RecordedCircuit(N)
    lwe.add_lwe_linear(0, [lwe.add_input(ValueKind.LWE0, np.zeros(1))], 1)
    for walk in (driver.run_circuit_by_handles, driver.push_circuit_by_handles):
        with pytest.raises(RuntimeError, match="add_glwe_poly_linear") as e:
            walk(None, rec)
        with pytest.raises(RuntimeError) as e_lwe:
            walk(None, lwe)
        assert str(e.value) == str(e_lwe.value).replace("add_lwe_linear", "add_glwe_poly_linear")


def test_the_slots_of_the_scattered_case_hold_what_they_are_for():
    for M, K in G.SCATTERED_SHAPES:
        for n in (16, 128, 2048):
            s = G.slots(M, K, n)
            off, exp, coef = s["general"][0]
            assert set(exp.tolist()) >= set(GC.seam_exponents(n)) and set(coef.tolist()) >= set(GC.EXTREME_COEFFICIENTS)
            assert int(off[1]) >= 8 and list(exp[int(off[1]) - 3:int(off[1])]) == [n - 1] * 3          # the exponent three times over
            if K >= 2:                                                   # the first tile is empty at k = K - 1
                assert all(off[m * K + K - 1] == off[m * K + K] for m in range(min(G.VT, M)))
            if M >= 2:                                                   # row 1 is empty
                assert off[K] == off[2 * K]
            assert s["general+bias"][1].shape == (M, n) and s["constants"][1] is None and s["empty+bias"][0][1].size == 0
    assert {m for m, _ in G.SCATTERED_SHAPES} == {1, G.VT, G.VT + 1, 2 * G.VT + 1} and {k % 4 for _, k in G.SCATTERED_SHAPES} == {0, 1, 2, 3}
    for K in (2, 4, 5, 7):
        pk = G.picks(G.LAYERS, K)
        assert all(p[0] in (5, 6) for p in pk) and pk[-1][-1] == pk[-1][0] and pk[0][0] == pk[2][0]  # one level; a repeat; a shared node
    assert G.picks(G.LAYERS, 1) == [[1], [0], [2]]


@pytest.mark.parametrize("a,b,s", G.MODEL_CASES)
def test_the_oracle_walks_the_decrypt_case_to_the_plaintext_model(a, b, s):
    """the condition of the GPU suite's decrypt-level case: with these keys and inputs, `poly_linear_ref` of the two packed
    integers under w = [X^s, 1], sample-extracted by the oracle, decrypts to the bits of (a << s) ^ b"""
    P, ks = G.keys_of("tuned")[:2]
    k1 = P.k + 1
    x = G.model_encrypt(P, ks, a, b)
    out = GC.poly_linear_ref(x.reshape(1, 2, k1, P.N), G.model_slot(s), 1, 2)[0, 0].reshape(-1)
    lwes = [O.sample_extract(out, j, P.N, P.k) for j in range(G.BITS + s)]
    assert G.model_decrypt(ks, lwes) == G.model(a, b, s)
    assert sum(bit << j for j, bit in enumerate(G.model(a, b, s))) == (a << s) ^ b
