"""The host side of the bootstraps by a caller's table and of the public functional keyswitch in gate graphs and by handle
(`SPF_OP_PBS_UNIVARIATE`, `SPF_OP_PBS_BIVARIATE`, `spf_graph_add_public_functional_keyswitch`): what needs no device.  A graph and
a pool need a context, and a context needs a device, so of the library's argument checks only the null handles can be reached
here; the others are in tests/test_gpu_pbs_graph.py and tests/test_gpu_pbs_by_handle.py.  `RecordedCircuit` records and refuses on
the host, and the last test shows that the GPU tests' comparison catches one flipped word."""
import ctypes as C

import numpy as np
import pytest

import spf_amd
from spf_amd import FheOp, ValueKind, _ffi
from spf_amd.graph import NODE_PUFKS, graph_op
from tests import pbs_graph_cases as K
from tests import pufks_cases as PC
from tests.polyref_cases import key_fft

N = 2048


def circuit():
    """(rec, lwe0 a, lwe0 b, lwe1, lut glwe1, ggsw1)"""
    rec = spf_amd.RecordedCircuit(N)
    a, b = rec.add_input(ValueKind.LWE0, np.zeros(1)), rec.add_input(ValueKind.LWE0, np.zeros(1))
    return (rec, a, b, rec.add_input(ValueKind.LWE1, np.zeros(1)), rec.add_input(ValueKind.GLWE1, np.zeros(1)),
            rec.add_input(ValueKind.GGSW1, np.zeros(1)))


def test_the_two_operations_have_the_headers_values():
    assert int(FheOp.PBS_UNIVARIATE) == 10 and int(FheOp.PBS_BIVARIATE) == 11 and NODE_PUFKS == 67
    assert graph_op(10) is FheOp.PBS_UNIVARIATE and graph_op(11) is FheOp.PBS_BIVARIATE and graph_op(9) is FheOp.MulXN
    assert len(list(FheOp)) == 10          # the reference's ten: the two bootstraps by table are no FheOp there


def test_entry_points_refuse_null_handles_without_a_device():
    lib = _ffi.load_library()
    nodes = (C.c_uint32 * 3)(0, 1, 2)
    out = C.c_uint32(7)
    assert lib.spf_graph_add_public_functional_keyswitch(None, nodes, 3, C.byref(out)) == 1 and out.value == 7
    for op, arity in ((FheOp.PBS_UNIVARIATE, 2), (FheOp.PBS_BIVARIATE, 3)):
        assert lib.spf_graph_add_op(None, int(op), nodes, arity, 0, C.byref(out)) == 1 and out.value == 7
        vals = (C.c_void_p * 3)()
        h, t = C.c_void_p(), C.c_uint64()
        assert lib.spf_pool_submit_op_v(None, int(op), vals, arity, 0, C.byref(h), C.byref(t)) == 1 and not h.value


def test_recorded_circuit_records_the_new_nodes():
    rec, a, b, l1, lut, _ = circuit()
    u = rec.add_op(FheOp.PBS_UNIVARIATE, [a, lut], 99)           # the parameter of a univariate bootstrap is forced to 0
    v = rec.add_op(FheOp.PBS_BIVARIATE, [a, a, lut], 63)         # f(x, x); 63 is the largest plaintext_bits
    w = rec.add_op(FheOp.PBS_BIVARIATE, [b, a, lut], 0)
    assert rec.op[u:] == [10, 11, 11] and rec.kind[u:] == [int(ValueKind.LWE1)] * 3 and rec.param[u:] == [0, 63, 0]
    assert rec.inputs[u:] == [(a, lut), (a, a, lut), (b, a, lut)]
    k1 = rec.add_public_functional_keyswitch([u, v, u, l1])     # lwe1 nodes of any origin; repeats allowed
    k0 = rec.add_public_functional_keyswitch([a])
    assert rec.op[k1:] == [NODE_PUFKS] * 2 and rec.kind[k1:] == [int(ValueKind.GLWE1)] * 2 and rec.param[k1:] == [4, 1]
    assert rec.inputs[k1:] == [(u, v, u, l1), (a,)]
    bits = rec.add_unpack(k1, 4)                                  # the new node is an ordinary GLWE1 node
    assert rec.add_public_functional_keyswitch(bits) == bits[-1] + 1
    rec.add_public_functional_keyswitch([a] * N)                  # lwe_count = N is accepted
    assert k0 == k1 + 1 and w == v + 1


def test_arrays_round_trip_a_circuit_holding_all_three():
    rec, a, b, l1, lut, _ = circuit()
    u = rec.add_op(FheOp.PBS_UNIVARIATE, [a, lut])
    v = rec.add_op(FheOp.PBS_BIVARIATE, [a, b, lut], 2)
    k = rec.add_public_functional_keyswitch([v, u, v])
    p = rec.add_pack([k, lut])
    k0 = rec.add_public_functional_keyswitch([b, a])
    rec.add_output(k, ValueKind.GLWE1)
    rec.add_output(rec.add_op(FheOp.MulXN, [k0], 3), ValueKind.GLWE1)
    arr = rec.arrays()
    assert list(arr["op"][u:]) == [10, 11, NODE_PUFKS, spf_amd.graph.NODE_PACK, NODE_PUFKS, int(FheOp.MulXN)]
    assert list(arr["n_in"][u:]) == [2, 3, 0, 0, 0, 1] and list(arr["n_bits"][u:]) == [0, 0, 3, 2, 2, 0]
    assert list(arr["ext_at"][[k, p, k0]]) == [0, 3, 5] and list(arr["ext"]) == [v, u, v, k, lut, b, a]
    assert int(arr["param"][v]) == 2
    again = spf_amd.RecordedCircuit.from_arrays(arr, rec.kind, rec.host, N)
    assert again.op == rec.op and again.kind == rec.kind and again.param == rec.param and again.inputs == rec.inputs
    assert again.outputs == rec.outputs


def test_recorded_circuit_refuses_what_the_library_refuses():
    rec, a, b, l1, lut, ggsw = circuit()
    n_nodes = len(rec.op)
    uni, biv, pufks = FheOp.PBS_UNIVARIATE, FheOp.PBS_BIVARIATE, rec.add_public_functional_keyswitch
    for call, word in [(lambda: rec.add_op(uni, [a]), "wrong number of operands"),
                       (lambda: rec.add_op(uni, [a, b, lut]), "wrong number of operands"),
                       (lambda: rec.add_op(biv, [a, lut]), "wrong number of operands"),
                       (lambda: rec.add_op(uni, [l1, lut]), "wrong ciphertext type"),
                       (lambda: rec.add_op(uni, [lut, a]), "wrong ciphertext type"),
                       (lambda: rec.add_op(uni, [a, ggsw]), "wrong ciphertext type"),
                       (lambda: rec.add_op(biv, [a, l1, lut]), "wrong ciphertext type"),
                       (lambda: rec.add_op(biv, [a, b, b]), "wrong ciphertext type"),
                       (lambda: rec.add_op(biv, [a, b, lut], 64), "plaintext_bits"),
                       (lambda: rec.add_op(biv, [a, b, lut], 1 << 40), "plaintext_bits"),
                       (lambda: rec.add_op(biv, [a, b, lut], -1), "plaintext_bits"),
                       (lambda: rec.add_op(uni, [a, n_nodes]), "not a node"),
                       (lambda: rec.add_op(biv, [a, b, n_nodes]), "not a node"),
                       (lambda: pufks([]), "lwe_count"),
                       (lambda: pufks([a] * (N + 1)), "lwe_count"),
                       (lambda: pufks([a, l1]), "mixed"),
                       (lambda: pufks([l1, l1, a]), "mixed"),
                       (lambda: pufks([lut]), "not an LWE"),
                       (lambda: pufks([a, ggsw]), "not an LWE"),
                       (lambda: pufks([a, n_nodes]), "not a node"),
                       (lambda: pufks([-1]), "not a node"),
                       (lambda: pufks([None]), "not a node")]:
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == 1 and word in str(e.value), str(e.value)
        assert len(rec.op) == n_nodes                                          # nothing recorded
    assert rec.add_op(biv, [a, b, lut], 63) == n_nodes and pufks([n_nodes]) == n_nodes + 1


def test_native_per_operation_drivers_say_that_they_cannot_walk_a_keyswitch_node():
    from tools import driver
    rec = spf_amd.RecordedCircuit(N)
    rec.add_public_functional_keyswitch([rec.add_input(ValueKind.LWE0, np.zeros(1))])
    for walk in (driver.run_circuit_by_handles, driver.push_circuit_by_handles):
        with pytest.raises(RuntimeError, match="add_public_functional_keyswitch"):
            walk(None, rec)


def test_the_comparison_bites():
    """the oracle's public functional keyswitch on the CPU; `same_words` accepts its own words, refuses one flipped bit in any
    word, another row order, a repeated row swapped for a fresh one, and another shape"""
    Nn, k, n, count, log, p = 128, 2, 7, 3, 4, 5
    key, lwes = PC.uniform_inputs(0x77, Nn, k, n, log, count, p)
    keyf = key_fft(key)
    want = PC.pufks_oracle(lwes, keyf, Nn, k, log, count)
    assert K.same_words(want, PC.pufks_oracle(lwes.copy(), keyf, Nn, k, log, count))
    for at in (0, want.size // 2, want.size - 1):
        got = want.copy()
        got.reshape(-1)[at] ^= np.uint64(1)
        assert not K.same_words(got, want), at
    assert not K.same_words(PC.pufks_oracle(lwes[::-1], keyf, Nn, k, log, count), want)
    assert not K.same_words(PC.pufks_oracle(lwes[[0, 1, 2, 3, 3]], keyf, Nn, k, log, count), want)
    assert not K.same_words(want.reshape(-1), want)
