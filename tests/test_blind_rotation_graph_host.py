"""The host side of blind rotation by an encrypted shift in gate graphs and by handle (`spf_graph_add_blind_rotation`,
`spf_pool_submit_blind_rotation_v`): what needs no device.  A graph and a pool need a context, and a context needs a device, so
of the library's argument checks only the null handles can be reached here; the others are in
tests/test_gpu_blind_rotation_graph.py and tests/test_gpu_blind_rotation_pool.py.  `RecordedCircuit` records and refuses on the
host, and the last test shows that the GPU tests' comparison catches each way the chain can be wrong."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import ValueKind, _ffi
from spf_amd.graph import NODE_ROT_CMUX
from tests import blind_rotation_graph_cases as K
from tests.util import random_glwe

P = O.DEFAULT_128


def test_entry_points_refuse_null_handles_without_a_device():
    lib = _ffi.load_library()
    nodes = (C.c_uint32 * 2)(0, 1)
    out = C.c_uint32(7)
    assert lib.spf_graph_add_blind_rotation(None, 0, nodes, 2, 0, C.byref(out)) == 1 and out.value == 7
    vals = (C.c_void_p * 2)()
    h, t = C.c_void_p(), C.c_uint64()
    assert lib.spf_pool_submit_blind_rotation_v(None, None, vals, 2, 0, C.byref(h), C.byref(t)) == 1 and not h.value


def test_recorded_circuit_records_one_node_per_bit():
    rec = spf_amd.RecordedCircuit(2048)
    sels = [rec.add_input(ValueKind.GGSW1, np.zeros(1)) for _ in range(3)]
    x = rec.add_input(ValueKind.GLWE1, np.zeros(1))
    last = rec.add_blind_rotation(x, sels, 4)
    assert last == 6 and len(rec.op) == 7
    assert rec.op[4:] == [NODE_ROT_CMUX] * 3 and rec.kind[4:] == [int(ValueKind.GLWE1)] * 3
    assert rec.param[4:] == [16, 32, 64]
    assert rec.inputs[4:] == [(sels[0], x), (sels[1], 4), (sels[2], 5)]       # (selector, accumulator): a chain
    assert rec.add_blind_rotation(last, [sels[1], sels[1]], 9) == 8            # repeats allowed; 2 + 9 = log2 N
    a = rec.arrays()
    assert list(a["op"][4:]) == [NODE_ROT_CMUX] * 5 and list(a["n_in"][4:]) == [2] * 5 and int(a["param"][8]) == 1024
    again = spf_amd.RecordedCircuit.from_arrays(a, rec.kind, rec.host, 2048)
    assert again.op == rec.op and again.param == rec.param and again.inputs == rec.inputs


def test_recorded_circuit_refuses_what_the_library_refuses():
    rec = spf_amd.RecordedCircuit(2048)
    sel = rec.add_input(ValueKind.GGSW1, np.zeros(1))
    x = rec.add_input(ValueKind.GLWE1, np.zeros(1))
    for call, word in [(lambda: rec.add_blind_rotation(x, []), "n_bits"),
                       (lambda: rec.add_blind_rotation(x, [sel] * 12), "n_bits + log_stride"),
                       (lambda: rec.add_blind_rotation(x, [sel, sel], 10), "n_bits + log_stride"),
                       (lambda: rec.add_blind_rotation(x, [sel], -1), "log_stride"),
                       (lambda: rec.add_blind_rotation(x, [sel, x]), "selector is not an L1 GGSW"),
                       (lambda: rec.add_blind_rotation(sel, [sel]), "operand is not an L1 GLWE"),
                       (lambda: rec.add_blind_rotation(2, [sel]), "not a node"),
                       (lambda: rec.add_blind_rotation(x, [2]), "not a node"),
                       (lambda: rec.add_blind_rotation(x, [None]), "not a node")]:
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == 1 and word in str(e.value), str(e.value)
        assert len(rec.op) == 2                                                # nothing recorded
    assert rec.add_blind_rotation(x, [sel], 10) == 2


def test_native_per_operation_drivers_say_that_they_cannot_walk_such_a_node():
    from tools import driver
    rec = spf_amd.RecordedCircuit(2048)
    rec.add_blind_rotation(rec.add_input(ValueKind.GLWE1, np.zeros(1)), [rec.add_input(ValueKind.GGSW1, np.zeros(1))])
    for walk in (driver.run_circuit_by_handles, driver.push_circuit_by_handles):
        with pytest.raises(RuntimeError, match="add_blind_rotation"):
            walk(None, rec)


def test_the_comparison_bites():
    """the oracle's chain on the CPU, and four wrong chains built from the oracle's own steps: the GPU tests' comparison
    (`same_words`) must refuse each of them"""
    n_bits, log_stride = 3, 2
    glwe, sels = random_glwe(0xBB0, 1, P.glwe_len)[0], K.random_selectors(0xBB1, n_bits, P)
    want = K.oracle_loop(glwe, sels, log_stride, P)
    assert K.same_words(want, K.oracle_loop(glwe, sels, log_stride, P))

    def chain(high, order=range(n_bits), stride=log_stride):
        acc = glwe
        for i in range(n_bits):
            acc = O.cmux(acc, high(acc, 1 << (i + stride)), sels[order[i]], P.N, P.k, P.cbs_radix_log, P.cbs_count)
        return acc

    def right(acc, r):
        return O.glwe_mul_xn(acc, 2 * P.N - r, P.N, P.k)

    def no_sign(acc, r):
        return np.roll(acc.reshape(P.k + 1, P.N), -r, axis=1).reshape(-1)

    assert K.same_words(want, chain(right))
    wrong = {"a rotation by r + 1": chain(lambda acc, r: right(acc, r + 1)),
             "no sign at the wrap": chain(no_sign),
             "selectors in descending order": chain(right, order=list(range(n_bits))[::-1]),
             "log_stride ignored": chain(right, stride=0)}
    for what, got in wrong.items():
        assert got.shape == want.shape and not K.same_words(got, want), what
    # the missing sign alone: the two chains differ only in the wrapped coefficients' sign, so even one step of r = 1 is caught
    one = O.cmux(glwe, no_sign(glwe, 1), sels[0], P.N, P.k, P.cbs_radix_log, P.cbs_count)
    assert not K.same_words(one, O.cmux(glwe, right(glwe, 1), sels[0], P.N, P.k, P.cbs_radix_log, P.cbs_count))
