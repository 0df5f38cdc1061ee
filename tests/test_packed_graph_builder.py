"""`RecordedCircuit` (the graph builder that is not bound to an executor) with the packed-integer node constructors
`add_unpack` / `add_pack`: what it records, that `arrays()` carries the new nodes and round-trips through `from_arrays`, and
the validation both builders share.  No GPU."""
import numpy as np
import pytest

import spf_amd
from spf_amd import FheOp, RecordedCircuit, ValueKind
from spf_amd.graph import NODE_PACK, NODE_UNPACK


def _circuit(N=16):
    g = RecordedCircuit(N)
    x = g.add_input(ValueKind.GLWE1, np.arange(2 * N, dtype=np.uint64))
    one = g.add_trivial(ValueKind.GLWE1, 1)
    bits = g.add_unpack(x, 3)
    rows = [g.add_op(FheOp.MultiplyGgswGlwe, [g.add_op(FheOp.CircuitBootstrap, [g.add_op(FheOp.KeyswitchL1toL0, [b])]), one])
            for b in bits]
    flipped = g.add_op(FheOp.Not, [rows[0]])
    p = g.add_pack(rows + [flipped, rows[0]])
    q = g.add_pack([p])
    g.add_output(q, ValueKind.GLWE1)
    g.add_output(bits[2], ValueKind.LWE1)
    return g, x, bits, rows, flipped, p, q


def test_builder_records_unpack_and_pack_nodes():
    g, x, bits, rows, flipped, p, q = _circuit()
    assert bits == [2, 3, 4]
    assert [g.op[b] for b in bits] == [NODE_UNPACK] * 3 and [g.param[b] for b in bits] == [0, 1, 2]
    assert all(g.kind[b] == ValueKind.LWE1 and g.inputs[b] == (x,) for b in bits)
    assert g.op[p] == NODE_PACK and g.kind[p] == ValueKind.GLWE1 and g.param[p] == 5
    assert g.inputs[p] == tuple(rows + [flipped, rows[0]]) and g.inputs[q] == (p,)


def test_arrays_carry_the_new_nodes_and_round_trip():
    g, x, bits, rows, flipped, p, q = _circuit()
    a = g.arrays()
    n = len(g.op)
    assert all(len(a[key]) == n for key in ("op", "in", "n_in", "param", "keep", "n_bits", "ext_at"))
    assert a["op"][bits].tolist() == [NODE_UNPACK] * 3 and a["n_bits"][bits].tolist() == [3, 3, 3]
    assert a["param"][bits].tolist() == [0, 1, 2] and a["n_in"][bits].tolist() == [1, 1, 1] and a["in"][bits, 0].tolist() == [x] * 3
    assert a["op"][p] == NODE_PACK and a["n_in"][p] == 0 and a["n_bits"][p] == 5 and a["n_bits"][q] == 1
    assert a["ext"][a["ext_at"][p]:a["ext_at"][p] + 5].tolist() == rows + [flipped, rows[0]]
    assert a["ext"][a["ext_at"][q]:a["ext_at"][q] + 1].tolist() == [p]
    assert len(a["ext"]) == 6 and not a["n_bits"][[x, rows[0], flipped]].any()
    assert sorted(np.flatnonzero(a["keep"]).tolist()) == sorted([q, bits[2]])

    h = RecordedCircuit.from_arrays(a, g.kind, g.host, 16)
    assert (h.op, h.kind, h.param, h.inputs) == (g.op, g.kind, g.param, g.inputs)
    assert sorted(h.outputs) == sorted(g.outputs)
    assert all((u is None) == (v is None) and (u is None or np.array_equal(u, v)) for u, v in zip(h.host, g.host))
    b = h.arrays()
    assert a.keys() == b.keys() and all(np.array_equal(a[key], b[key]) for key in a)
    # a circuit without the new nodes keeps the arrays it had, plus empty extensions
    plain = RecordedCircuit()
    y = plain.add_input(ValueKind.GLWE1, np.zeros(4096, dtype=np.uint64))
    plain.add_output(plain.add_op(FheOp.Not, [y]), ValueKind.GLWE1)
    c = plain.arrays()
    assert c["op"].tolist() == [-1, int(FheOp.Not)] and c["n_in"].tolist() == [0, 1] and len(c["ext"]) == 0 and not c["n_bits"].any()


def test_builder_validation():
    g = RecordedCircuit(16)
    x = g.add_input(ValueKind.GLWE1, np.zeros(32, dtype=np.uint64))
    lwe = g.add_input(ValueKind.LWE1, np.zeros(17, dtype=np.uint64))
    before = len(g.op)
    for bad in (0, -1, 17, 1.5, True, None):
        with pytest.raises(spf_amd.SpfError):
            g.add_unpack(x, bad)
    for node in (lwe, 99, -1, None):
        with pytest.raises(spf_amd.SpfError):
            g.add_unpack(node, 2)
    for rows in ([], [x] * 17, [x, lwe], [x, 99], [x, -1], [None]):
        with pytest.raises(spf_amd.SpfError):
            g.add_pack(rows)
    assert len(g.op) == before                                    # a refused call recorded nothing
    assert len(g.add_unpack(x, 16)) == 16 and g.add_pack([x] * 16) == before + 16
    with pytest.raises(spf_amd.SpfError):
        g.add_pack([g.add_unpack(x, 1)[0]])                       # an unpacked bit is an LWE


def test_executor_binding_validates_before_calling_the_library():
    """FheCircuit.add_unpack / add_pack check n_bits and the ids' type in Python: no handle is needed to be refused"""
    from spf_amd.graph import FheCircuit

    class _Params:
        polynomial_degree = 16

    class _Eng:
        params = _Params()

    g = FheCircuit.__new__(FheCircuit)
    g._eng, g._lib, g._g = _Eng(), None, None
    for bad in (0, 17, -3, 2.0, None):
        with pytest.raises(spf_amd.SpfError):
            g.add_unpack(0, bad)
    for node in (-1, 1 << 32, "0", None):
        with pytest.raises(spf_amd.SpfError):
            g.add_unpack(node, 2)
    for rows in ([], [0] * 17, [0, -1], [0, None], [1 << 32]):
        with pytest.raises(spf_amd.SpfError):
            g.add_pack(rows)


def test_graph_builder_forwards_the_packed_nodes_to_a_recorded_circuit():
    """`mux_circuits.GraphBuilder` over a RecordedCircuit: an 8-bit adder block fed by two packed integers and packed again;
    the recording carries one unpack per integer and one pack through `arrays()`"""
    from spf_amd.mux_circuits import GraphBuilder, ripple_carry_adder
    rec = RecordedCircuit(2048)
    b = GraphBuilder(rec)
    xa = rec.add_input(ValueKind.GLWE1, np.zeros(4096, dtype=np.uint64))
    xb = rec.add_input(ValueKind.GLWE1, np.ones(4096, dtype=np.uint64))
    ga, gb = ([rec.add_op(FheOp.CircuitBootstrap, [rec.add_op(FheOp.KeyswitchL1toL0, [x])]) for x in b.add_unpack(src, 8)]
              for src in (xa, xb))
    assert all(rec.op[n] == int(FheOp.CircuitBootstrap) for n in ga + gb)
    sums = b.insert(ripple_carry_adder(8, 8, False), [x for pair in zip(ga, gb) for x in pair])
    assert len(sums) == 9
    out = b.add_pack(sums)
    rec.add_output(out, ValueKind.GLWE1)
    assert b.add_unpack(out, 9) == list(range(out + 1, out + 10))   # a packed result can be taken apart again
    a = rec.arrays()
    assert int((a["op"] == NODE_UNPACK).sum()) == 8 + 8 + 9 and int((a["op"] == NODE_PACK).sum()) == 1
    assert int((a["op"] == int(FheOp.SampleExtract)).sum()) == 0
    assert a["ext"].tolist() == list(sums) and a["keep"][out] == 1
    h = RecordedCircuit.from_arrays(a, rec.kind, rec.host)
    assert (h.op, h.param, h.inputs) == (rec.op, rec.param, rec.inputs)
