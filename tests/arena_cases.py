"""The three circuits the arena planner is held to (tests/test_arena_plan.py), recorded with `spf_amd.mux_circuits`, and their
group lists as the planner takes them."""
import os

import numpy as np

import spf_amd
from spf_amd import ValueKind
from spf_amd.gate_pool import circuit_jobs_as_one_graph
from spf_amd.graph import NODE_PACK, NODE_UNPACK, RecordedCircuit
from spf_amd.mux_circuits import GraphBuilder, append_uint_multiply, parse_mux_circuit, ripple_carry_adder

DATA = os.path.join(os.path.dirname(spf_amd.__file__), "data")
NEVER = 0xFFFFFFFF

# arena_bytes may be at most this fraction of values_bytes (numerator, denominator)
BOUNDS = {"add32": (1, 2), "mul8": (1, 4), "mul32": (1, 8)}


def _block(n):
    return parse_mux_circuit(open(os.path.join(DATA, f"mux_multiplier_n{n}_m{n}.bincode"), "rb").read())


def record(name: str, P=spf_amd.DEFAULT_128) -> RecordedCircuit:
    """add32: `ripple_carry_adder(32, 32)` fed as `add_circuit` does; mul8: the 8 x 8 multiplier block fed the same way;
    mul32: 32 x 32 via `append_uint_multiply`.  Every input is the same dummy GLWE: only the shape matters here."""
    dummy = np.zeros(P.glwe_words, dtype=np.uint64)
    if name == "add32":
        bits = np.broadcast_to(dummy, (1, 64, P.glwe_words))
        return circuit_jobs_as_one_graph(None, ripple_carry_adder(32, 32, False), bits, record=True)[0]
    if name == "mul8":
        bits = np.broadcast_to(dummy, (1, 16, P.glwe_words))
        return circuit_jobs_as_one_graph(None, _block(8), bits, record=True)[0]
    assert name == "mul32"
    blk16 = _block(16)
    g = RecordedCircuit(P.polynomial_degree)
    b = GraphBuilder(g)
    sel = [b.to_ggsw(g.add_input(ValueKind.GLWE1, dummy)) for _ in range(64)]
    for n in append_uint_multiply(b, sel[:32], sel[32:], lambda x, y: {(16, 16): blk16}[(x, y)]):
        g.add_output(n, ValueKind.GLWE1)
    return g


def value_bytes(P, kind: int) -> int:
    return 8 * {ValueKind.LWE0: P.lwe0_words, ValueKind.LWE1: P.lwe1_words, ValueKind.GLWE1: P.glwe_words,
                ValueKind.GGSW1: 2 * P.cbs_ggsw_complex, ValueKind.GLEV1: P.cbs_radix_count * P.glwe_words}[ValueKind(kind)]


def values_bytes(rec: RecordedCircuit, P) -> int:
    """the input region (inputs and constants, each on 256 bytes) plus the size of every other node's value"""
    region = sum(-(-value_bytes(P, k) // 256) * 256 for o, k in zip(rec.op, rec.kind) if o < 0)
    return region + sum(value_bytes(P, k) for o, k in zip(rec.op, rec.kind) if o >= 0)


def group_list(rec: RecordedCircuit, P):
    """-> (base, [(level, row_bytes, [death per row])]): ASAP levels, one group per (level, operation, parameter) with members
    in node order, groups ordered by that key; a row dies at the level of its last reader, an output never."""
    n = len(rec.op)
    level = [0] * n
    death = [0] * n
    for i in range(n):
        if rec.op[i] >= 0:
            level[i] = 1 + max(level[j] for j in rec.inputs[i])
        death[i] = level[i]
        for j in rec.inputs[i]:
            death[j] = max(death[j], level[i])
    for o in rec.outputs:
        death[o] = NEVER
    base = sum(-(-value_bytes(P, k) // 256) * 256 for o, k in zip(rec.op, rec.kind) if o < 0)
    groups = {}
    for i in range(n):
        if rec.op[i] < 0:
            continue
        if rec.op[i] == NODE_UNPACK:
            param = rec._unpack_width[i]
        elif rec.op[i] == NODE_PACK:
            param = len(rec.inputs[i])
        else:
            param = rec.param[i]
        groups.setdefault((level[i], rec.op[i], param), []).append(i)
    out = []
    for key in sorted(groups):
        members = groups[key]
        out.append((key[0], value_bytes(P, rec.kind[members[0]]), [death[i] for i in members]))
    return base, out


def write_group_list(path, base, groups):
    with open(path, "w") as f:
        f.write(f"{base} {len(groups)}\n")
        for level, row_bytes, deaths in groups:
            f.write(f"{level} {row_bytes} {len(deaths)} " + " ".join(map(str, deaths)) + "\n")
