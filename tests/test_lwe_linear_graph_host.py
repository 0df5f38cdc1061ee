"""The host side of the plaintext linear maps over LWE ciphertexts as gate-graph nodes (`spf_graph_add_lwe_linear`,
`spf_lwe_linear_slot_shape`): what needs no device.  A graph needs a context and a context needs a device, so of the library's
argument checks only the null handles can be reached here; the others are in tests/test_gpu_lwe_linear_graph.py.
`RecordedCircuit` records and refuses on the host, and the last test is the condition of the GPU suite's decrypt-level case: the
ORACLE's walk of those exact inputs decrypts to the plaintext model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spf_amd
from spf_amd import FheOp, ValueKind, _ffi
from spf_amd.graph import NODE_LWE_LINEAR
from tests import lwe_linear_cases as LC
from tests import lwe_linear_graph_cases as G

N = 2048
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def circuit():
    """(rec, lwe0 a, lwe0 b, lwe1, glwe1, ggsw1)"""
    rec = spf_amd.RecordedCircuit(N)
    a, b = rec.add_input(ValueKind.LWE0, np.zeros(1)), rec.add_input(ValueKind.LWE0, np.zeros(1))
    return (rec, a, b, rec.add_input(ValueKind.LWE1, np.zeros(1)), rec.add_input(ValueKind.GLWE1, np.zeros(1)),
            rec.add_input(ValueKind.GGSW1, np.zeros(1)))


def test_the_node_kind_is_68_and_is_a_NODE_name():
    """a NODE_* name: the random differential tests of gate graphs draw every one of them (tests/test_graph_fuzz_host.py)"""
    import spf_amd.graph as graph
    assert NODE_LWE_LINEAR == 68
    assert [n for n in dir(graph) if n.startswith("NODE_") and getattr(graph, n) == 68] == ["NODE_LWE_LINEAR"]
    assert graph.LWE_LINEAR_SLOTS == G.SLOTS and graph.LWE_LINEAR_GRAPH_MAX_ROWS == G.MAX_ROWS


def test_the_header_declares_and_the_binding_binds_both_symbols():
    with open(os.path.join(ROOT, "include", "spf_hip.h")) as f:
        header = f.read()
    assert re.search(r"spf_status spf_lwe_linear_slot_shape\(spf_ctx \*ctx, uint32_t slot, size_t \*M, size_t \*K, int \*has_bias\);", header)
    assert re.search(r"spf_status spf_graph_add_lwe_linear\(spf_graph \*graph, uint32_t slot, const uint32_t \*lwe_nodes", header)
    assert re.search(r"SPF_GRAPH_LWE_LINEAR_MAX_ROWS = %d\b" % G.MAX_ROWS, header)
    assert re.search(r"SPF_LWE_LINEAR_SLOTS = %d\b" % G.SLOTS, header)
    lib = _ffi.load_library()
    assert lib.spf_graph_add_lwe_linear.argtypes is not None and len(lib.spf_graph_add_lwe_linear.argtypes) == 6
    assert lib.spf_lwe_linear_slot_shape.argtypes is not None and len(lib.spf_lwe_linear_slot_shape.argtypes) == 5
    assert callable(spf_amd.Engine.lwe_linear_slot_shape) and callable(spf_amd.FheCircuit.add_lwe_linear)
    assert callable(spf_amd.RecordedCircuit.add_lwe_linear)


def test_entry_points_refuse_null_handles_without_a_device():
    lib = _ffi.load_library()
    nodes = (C.c_uint32 * 3)(0, 1, 2)
    out = (C.c_uint32 * 2)(7, 7)
    assert lib.spf_graph_add_lwe_linear(None, 0, nodes, 3, 2, out) == 1 and list(out) == [7, 7]
    M, K, has_bias = C.c_size_t(5), C.c_size_t(5), C.c_int(5)
    assert lib.spf_lwe_linear_slot_shape(None, 0, C.byref(M), C.byref(K), C.byref(has_bias)) == 1
    assert (M.value, K.value, has_bias.value) == (5, 5, 5)


def test_recorded_circuit_records_a_layer_as_m_nodes_over_one_operand_list():
    rec, a, b, l1, glwe, _ = circuit()
    bits = rec.add_unpack(glwe, 2)                                   # lwe1 nodes one level up
    rows = rec.add_lwe_linear(5, [l1, bits[1], l1], 4)               # lwe1 nodes of any origin; repeats allowed
    assert rows == list(range(bits[-1] + 1, bits[-1] + 5))
    assert rec.op[rows[0]:] == [NODE_LWE_LINEAR] * 4 and rec.kind[rows[0]:] == [int(ValueKind.LWE1)] * 4
    assert rec.param[rows[0]:] == [0, 1, 2, 3] and rec.inputs[rows[0]:] == [(l1, bits[1], l1)] * 4
    low = rec.add_lwe_linear(63, [a], 1)                             # one operand, one row, the last slot; lwe0 in, lwe0 out
    assert rec.kind[low[0]] == int(ValueKind.LWE0)
    ks = rec.add_op(FheOp.KeyswitchL1toL0, [rows[3]])                # the new nodes are ordinary LWE nodes
    again = rec.add_lwe_linear(0, [ks, a, low[0]], 2)
    assert len(rec.add_lwe_linear(0, [a], G.MAX_ROWS)) == G.MAX_ROWS  # M at the limit is accepted
    lv = G.levels(rec)
    assert [lv[n] for n in rows] == [2] * 4                          # one level above the highest operand (the unpack bits: 1)
    assert [lv[n] for n in low] == [1] and [lv[n] for n in again] == [4, 4]


def test_arrays_carry_the_layer_and_round_trip():
    rec, a, b, l1, glwe, _ = circuit()
    p = rec.add_public_functional_keyswitch([b, a])
    rows = rec.add_lwe_linear(9, [b, a, b], 2)
    more = rec.add_lwe_linear(10, rows, 3)
    k = rec.add_pack([p, glwe])
    rec.add_output(more[2], ValueKind.LWE0)
    rec.add_output(rows[0], ValueKind.LWE0)
    arr = rec.arrays()
    at = rows[0]
    assert list(arr["op"][at:at + 5]) == [NODE_LWE_LINEAR] * 5 and list(arr["n_in"][at:at + 5]) == [0] * 5
    assert list(arr["n_bits"][at:at + 5]) == [3, 3, 2, 2, 2] and list(arr["param"][at:at + 5]) == [0, 1, 0, 1, 2]
    assert list(arr["lin_slot"][at:at + 5]) == [9, 9, 10, 10, 10] and list(arr["lin_rows"][at:at + 5]) == [2, 2, 3, 3, 3]
    # the operand lists in node order, ONE per layer: [pufks | layer 9 | layer 10 | pack]
    assert list(arr["ext"]) == [b, a, b, a, b, rows[0], rows[1], p, glwe]
    assert list(arr["ext_at"][[p, rows[0], rows[1], more[0], more[2], k]]) == [0, 2, 2, 5, 5, 7]
    assert arr["lin_rows"][p] == 0 and arr["lin_rows"][k] == 0 and list(np.flatnonzero(arr["keep"])) == [rows[0], more[2]]
    again = spf_amd.RecordedCircuit.from_arrays(arr, rec.kind, rec.host, N)
    assert again.op == rec.op and again.kind == rec.kind and again.param == rec.param and again.inputs == rec.inputs
    assert again._linear == rec._linear and sorted(again.outputs) == sorted(rec.outputs)


def test_recorded_circuit_refuses_what_the_library_refuses():
    rec, a, b, l1, glwe, ggsw = circuit()
    n_nodes = len(rec.op)
    lin = rec.add_lwe_linear
    for call, word in [(lambda: lin(G.SLOTS, [a], 1), "slot"),
                       (lambda: lin(-1, [a], 1), "slot"),
                       (lambda: lin(None, [a], 1), "slot"),
                       (lambda: lin(True, [a], 1), "slot"),
                       (lambda: lin(0, [], 1), "K = 0"),
                       (lambda: lin(0, [a], 0), "M must be"),
                       (lambda: lin(0, [a], G.MAX_ROWS + 1), "M must be"),
                       (lambda: lin(0, [a], None), "M must be"),
                       (lambda: lin(0, [a], 1.0), "M must be"),
                       (lambda: lin(0, [a, l1], 1), "mixed"),
                       (lambda: lin(0, [l1, l1, a], 1), "mixed"),
                       (lambda: lin(0, [glwe], 1), "not an LWE"),
                       (lambda: lin(0, [a, ggsw], 1), "not an LWE"),
                       (lambda: lin(0, [a, n_nodes], 1), "not a node"),
                       (lambda: lin(0, [-1], 1), "not a node"),
                       (lambda: lin(0, [None], 1), "not a node")]:
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == 1 and word in str(e.value), str(e.value)
        assert len(rec.op) == n_nodes                                          # nothing recorded
    assert lin(0, [a, b], 2) == [n_nodes, n_nodes + 1]


def test_the_builder_of_mux_circuits_passes_the_layer_on():
    from spf_amd.mux_circuits import GraphBuilder
    rec, a, b, l1, _, _ = circuit()
    rows = GraphBuilder(rec).add_lwe_linear(3, [a, b], 2)
    assert rec.op[rows[0]:] == [NODE_LWE_LINEAR] * 2 and rec._linear[rows[1]] == (3, 2)


def test_native_per_operation_drivers_say_that_they_cannot_walk_a_linear_node():
    from tools import driver
    rec = spf_amd.RecordedCircuit(N)
    rec.add_lwe_linear(0, [rec.add_input(ValueKind.LWE0, np.zeros(1))], 1)
    for walk in (driver.run_circuit_by_handles, driver.push_circuit_by_handles):
        with pytest.raises(RuntimeError, match="add_lwe_linear"):
            walk(None, rec)


def test_the_hard_weights_hold_what_they_are_for():
    w = G.HARD_WEIGHTS
    assert w.shape == (3, 4) and LC.limbs_of(int(w.min()), int(w.max())) == 0
    for v in (LC.INT64_MIN, LC.INT64_MAX, -1, 0, 1) + LC.FIRST_BEYOND:
        assert (w == v).any(), v
    x = LC.uniform_inputs(0xECF0, 1, 4, 5)[0]
    assert np.array_equal(LC.linear_ref(x, w), np.array(LC.linear_literal(x, w), dtype=np.uint64))


def test_the_oracle_walks_the_decrypt_case_to_the_plaintext_model():
    """the condition of test_the_chain_decrypts_to_the_plaintext_model: with these keys, inputs, weights and tables the oracle's
    own chain decrypts to the model's answer, in both runs — and every intermediate carries its message"""
    P, ks = G.keys_of("tuned")[:2]
    lut1, lut2 = G.model_tables(P)
    assert [G.model(x) for x in G.MODEL_INPUTS] == [[0, 1], [1, 2]]
    for run in range(2):
        x = G.model_encrypt(ks, run)
        got = G.chain_by_oracle(P, ks, ValueKind.LWE0, x, G.MODEL_WA, G.model_bias_words(), G.MODEL_WB, None, lut1, lut2)
        assert G.model_decrypt(ks, got["y"]) == G.model(G.MODEL_INPUTS[run]), run
        a = [int(LC.lwe_phases(r, ks.lwe_sk)) for r in got["a"]]
        h = [int(LC.lwe_phases(r, ks.glwe_sk)) for r in got["h"]]
        assert [((v + (1 << 59)) >> 60) & 15 for v in a] == [[4, 1, 5], [4, 4, 2]][run]       # layer A, 3 bits under the padding bit
        assert [((v + (1 << 60)) >> 61) & 7 for v in h] == [[1, 0, 2], [1, 1, 1]][run]       # table 1's results = layer B's messages
