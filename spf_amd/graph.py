"""Host-side mirror of ``FheCircuit`` + ``CircuitProcessor::run_graph_blocking`` over the graph
executor of the C ABI (``spf_graph_*``, include/spf_hip.h; spf_amd/csrc/spf_graph.hpp).

The reference builds a petgraph DAG of ``FheOp`` nodes joined by typed ``FheEdge``s
(parasol_runtime/src/fhe_circuit.rs:34-205) and runs it with one rayon task per node
(circuit_processor/mod.rs:130-253, 573-623).  Here the same DAG is handed to the library, which runs
it level by level as batched launches with every intermediate in HBM.
"""
from __future__ import annotations

import ctypes as C
import enum
from typing import List, Sequence

import numpy as np

from ._ffi import Engine, SpfError, _ptr


class ValueKind(enum.IntEnum):
    LWE0 = 0
    LWE1 = 1
    GLWE1 = 2
    GGSW1 = 3
    GLEV1 = 4


class FheOp(enum.IntEnum):
    """The computing variants of ``FheOp`` (fhe_circuit.rs:65-126); inputs, outputs and constants have
    their own methods on :class:`FheCircuit`."""
    SampleExtract = 0
    KeyswitchL1toL0 = 1
    Not = 2
    GlweAdd = 3
    CMux = 4
    GlevCMux = 5
    MultiplyGgswGlwe = 6
    CircuitBootstrap = 7
    SchemeSwitch = 8
    MulXN = 9


class TableOp(enum.IntEnum):
    """The `spf_graph_op` values that are no `FheOp` of the reference: `programmable_bootstrap_univariate` / `_bivariate`
    (programmable_bootstrapping.rs:291, 575-621) with the lookup table as the last operand, a GLWE1 node; PBS_BIVARIATE's param
    is plaintext_bits (< 64).  Taken wherever an FheOp is (`add_op`, `Pool.submit_v` / `push_v` / `run_v`) and reachable as
    `FheOp.PBS_UNIVARIATE` / `FheOp.PBS_BIVARIATE`; iterating `FheOp` still gives the reference's ten."""
    PBS_UNIVARIATE = 10
    PBS_BIVARIATE = 11


FheOp.PBS_UNIVARIATE = TableOp.PBS_UNIVARIATE
FheOp.PBS_BIVARIATE = TableOp.PBS_BIVARIATE


class KeyswitchOp(enum.IntEnum):
    """Three more `spf_graph_op` values that are no `FheOp` of the reference: `keyswitch_glwe_to_glwe` (fft_ops.rs:457-495) under
    the key of slot `param`, round `param` (1 .. log2 N) of the trace's loop, and `trace` (ops/automorphisms/mod.rs:53-85); one GLWE1
    operand, one GLWE1 result.  Taken wherever an FheOp is and reachable as `FheOp.GLWE_KEYSWITCH` / `GLWE_AUTOMORPHISM` /
    `GLWE_TRACE`.  In a gate graph they are the nodes of `add_glwe_keyswitch` / `add_glwe_automorphism` / `add_glwe_trace`
    (NODE_GLWE_KEYSWITCH .. NODE_GLWE_TRACE below: `add_op` records them as those nodes, whichever door built them).  An enum of
    its own, beside TableOp: the values 12 .. 14 never stand in a recorded circuit, so the random graph generator of the
    differential tests, which draws every member of FheOp and TableOp as a node, draws these three as the NODE_* constants."""
    GLWE_KEYSWITCH = 12
    GLWE_AUTOMORPHISM = 13
    GLWE_TRACE = 14


FheOp.GLWE_KEYSWITCH = KeyswitchOp.GLWE_KEYSWITCH
FheOp.GLWE_AUTOMORPHISM = KeyswitchOp.GLWE_AUTOMORPHISM
FheOp.GLWE_TRACE = KeyswitchOp.GLWE_TRACE


def graph_op(op):
    """the member of FheOp, TableOp or KeyswitchOp that a `spf_graph_op` value names"""
    for extra in (TableOp, KeyswitchOp):
        if int(op) in extra._value2member_map_:
            return extra(op)
    return FheOp(op)


# RecordedCircuit's codes of the node constructors that are no FheOp (spf_graph_add_unpack / spf_graph_add_pack /
# spf_graph_add_blind_rotation: one NODE_ROT_CMUX per bit, inputs (selector, accumulator), param = the rotation /
# spf_graph_add_public_functional_keyswitch: inputs = all lwe_count operands, param = lwe_count)
NODE_UNPACK = 64
NODE_PACK = 65
NODE_ROT_CMUX = 66
NODE_PUFKS = 67
# spf_graph_add_lwe_linear: one node per output row m, inputs = all K operands (one list shared by the M nodes of a call), param = m
NODE_LWE_LINEAR = 68
LWE_LINEAR_NODE = NODE_LWE_LINEAR  # its name in the revision before: that revision's test modules import it and must still load
LWE_LINEAR_SLOTS = 64            # SPF_LWE_LINEAR_SLOTS
LWE_LINEAR_GRAPH_MAX_ROWS = 4096  # SPF_GRAPH_LWE_LINEAR_MAX_ROWS
# spf_graph_add_glwe_poly_linear: one GLWE1 node per output row m, inputs = all K operands (one list shared by the M nodes of a
# call), param = m.  A NODE_* name: the random graph generator of the differential tests draws every NODE_* of this module, and it
# draws the polynomial weights apart from the circuit (tests/graph_fuzz_cases.py, draw_glwe_poly_slots).
NODE_GLWE_POLY_LINEAR = 69
GLWE_POLY_LINEAR_NODE = NODE_GLWE_POLY_LINEAR  # its name in the revisions before: their test modules and tools import it
GLWE_POLY_SLOTS = 64       # SPF_GLWE_POLY_SLOTS
GLWE_POLY_MAX_ROWS = 4096  # SPF_GLWE_POLY_MAX_ROWS
_LINEAR_NODES = (NODE_LWE_LINEAR, NODE_GLWE_POLY_LINEAR)   # M nodes over one operand list, with a weight slot
# spf_graph_add_glwe_keyswitch / _automorphism / _trace: one GLWE1 node over one GLWE1 operand, param = the keyswitch-key slot / the
# round / 0.  NODE_* names as well: the generator draws the keyswitch keys apart from the circuit (draw_glwe_ksk_slots)
NODE_GLWE_KEYSWITCH = 70
NODE_GLWE_AUTOMORPHISM = 71
NODE_GLWE_TRACE = 72
GLWE_KEYSWITCH_NODE, GLWE_AUTOMORPHISM_NODE, GLWE_TRACE_NODE = NODE_GLWE_KEYSWITCH, NODE_GLWE_AUTOMORPHISM, NODE_GLWE_TRACE  # (likewise)
GLWE_KSK_SLOTS = 16   # SPF_GLWE_KSK_SLOTS
_GLWE_KS_NODES = (GLWE_KEYSWITCH_NODE, GLWE_AUTOMORPHISM_NODE, GLWE_TRACE_NODE)
# ... which spf_graph_add_op records for the three KeyswitchOp values as well (the same node, whichever door built it)
_GLWE_KS_NODE_OF = {int(KeyswitchOp.GLWE_KEYSWITCH): GLWE_KEYSWITCH_NODE, int(KeyswitchOp.GLWE_AUTOMORPHISM): GLWE_AUTOMORPHISM_NODE,
                    int(KeyswitchOp.GLWE_TRACE): GLWE_TRACE_NODE}
_GLWE_KS_NAME = {GLWE_KEYSWITCH_NODE: "add_glwe_keyswitch", GLWE_AUTOMORPHISM_NODE: "add_glwe_automorphism", GLWE_TRACE_NODE: "add_glwe_trace"}

# operand kinds of the operations whose arguments RecordedCircuit checks itself, as the library's table does (spf_ops.hpp)
_PBS_IN_KINDS = {int(TableOp.PBS_UNIVARIATE): (0, 2), int(TableOp.PBS_BIVARIATE): (0, 0, 2)}


def _check_lwe_count(what: str, lwe_count: int, degree: int) -> int:
    if not 0 < lwe_count <= degree:
        raise SpfError(1, f"{what}: lwe_count must be in 1 ..= {degree}, got {lwe_count!r}")
    return int(lwe_count)


def _check_n_bits(what: str, n_bits: int, degree: int) -> int:
    if isinstance(n_bits, bool) or not isinstance(n_bits, (int, np.integer)) or not 0 < n_bits <= degree:
        raise SpfError(1, f"{what}: n_bits must be in 1 ..= {degree}, got {n_bits!r}")
    return int(n_bits)


def _check_blind_rotation(what: str, n_bits: int, log_stride, degree: int) -> int:
    log_n = degree.bit_length() - 1
    if isinstance(log_stride, bool) or not isinstance(log_stride, (int, np.integer)) or log_stride < 0:
        raise SpfError(1, f"{what}: log_stride must be a non-negative integer, got {log_stride!r}")
    if n_bits < 1:
        raise SpfError(1, f"{what}: n_bits must be at least 1")
    if n_bits + log_stride > log_n:
        raise SpfError(1, f"{what}: n_bits + log_stride above log2(polynomial_degree) = {log_n}")
    return int(log_stride)


def _check_lwe_linear(what: str, slot, n_operands: int, M, slots: int = LWE_LINEAR_SLOTS, max_rows: int = LWE_LINEAR_GRAPH_MAX_ROWS) -> tuple:
    """slot, K and M of a linear layer (add_lwe_linear; add_glwe_poly_linear with its own limits)"""
    if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= slot < slots:
        raise SpfError(1, f"{what}: slot must be in 0 .. {slots - 1}, got {slot!r}")
    if n_operands < 1:
        raise SpfError(1, f"{what}: K = 0 operands")
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or not 0 < M <= max_rows:
        raise SpfError(1, f"{what}: M must be in 1 ..= {max_rows}, got {M!r}")
    return int(slot), int(M)


def _check_glwe_ks(what: str, op: int, param, degree: int) -> int:
    """the slot of add_glwe_keyswitch, the round of add_glwe_automorphism (add_glwe_trace has no parameter)"""
    if op == GLWE_TRACE_NODE:
        return 0
    if isinstance(param, bool) or not isinstance(param, (int, np.integer)):
        raise SpfError(1, f"{what}: {param!r} is not an integer")
    if op == GLWE_KEYSWITCH_NODE and not 0 <= param < GLWE_KSK_SLOTS:
        raise SpfError(1, f"{what}: slot must be in 0 .. {GLWE_KSK_SLOTS - 1}, got {param!r}")
    log_n = degree.bit_length() - 1
    if op == GLWE_AUTOMORPHISM_NODE and not 1 <= param <= log_n:
        raise SpfError(1, f"{what}: round {param!r} outside 1 .. log2 N = {log_n}")
    return int(param)


def _check_node(what: str, node, n_nodes: int) -> int:
    if isinstance(node, bool) or not isinstance(node, (int, np.integer)) or not 0 <= node < n_nodes:
        raise SpfError(1, f"{what}: {node!r} is not a node of this circuit")
    return int(node)


class FheCircuit:
    def __init__(self, engine: Engine):
        self._eng = engine
        self._lib = engine._lib
        h = C.c_void_p()
        from ._ffi import Group
        if isinstance(engine, Group):   # a job of the group: placed on a member when it is run (Group.run_graphs / run())
            engine._ck(engine._raw.spf_group_graph_create(engine._h, C.byref(h)))
            self._lib = engine._raw
        else:
            engine._ck(self._lib.spf_graph_create(engine._h, C.byref(h)))
        self._g = h
        self._keep: List[np.ndarray] = []   # input / output buffers the library reads and writes at run()

    def close(self):
        if getattr(self, "_g", None):
            self._lib.spf_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _words(self, kind: ValueKind) -> int:
        p = self._eng.params
        return {ValueKind.LWE0: p.lwe0_words, ValueKind.LWE1: p.lwe1_words, ValueKind.GLWE1: p.glwe_words,
                ValueKind.GGSW1: 2 * p.cbs_ggsw_complex,
                ValueKind.GLEV1: p.cbs_radix_count * p.glwe_words}[ValueKind(kind)]

    # FheOp::Input* — the array is read at every run(); change its contents to re-run on new data
    def add_input(self, kind: ValueKind, value: np.ndarray) -> int:
        a = np.ascontiguousarray(value)
        if a.nbytes != self._words(kind) * 8:
            raise SpfError(1, f"input of kind {ValueKind(kind).name} must have {self._words(kind) * 8} bytes, got {a.nbytes}")
        self._keep.append(a)
        node = C.c_uint32()
        self._eng._ck(self._lib.spf_graph_add_input(self._g, int(kind), _ptr(a), C.byref(node)))
        return node.value

    # FheOp::{Zero,One}{Lwe0,Glwe1,Glev1,Ggsw1} (fhe_circuit.rs:96-116)
    def add_trivial(self, kind: ValueKind, bit: int) -> int:
        node = C.c_uint32()
        self._eng._ck(self._lib.spf_graph_add_trivial(self._g, int(kind), bit, C.byref(node)))
        return node.value

    def add_op(self, op: FheOp, inputs: Sequence[int], param: int = 0) -> int:
        arr = (C.c_uint32 * len(inputs))(*inputs)
        node = C.c_uint32()
        self._eng._ck(self._lib.spf_graph_add_op(self._g, int(op), arr, len(inputs), param, C.byref(node)))
        return node.value

    # PackedGenericInt::graph_input(ctx).unpack(ctx): n_bits LWE1 nodes, node i = SampleExtract(i) of the packed GLWE1 node
    def add_unpack(self, glwe_node: int, n_bits: int) -> List[int]:
        n_bits = _check_n_bits("add_unpack", n_bits, self._eng.params.polynomial_degree)
        if isinstance(glwe_node, bool) or not isinstance(glwe_node, (int, np.integer)) or not 0 <= glwe_node < 1 << 32:
            raise SpfError(1, f"add_unpack: {glwe_node!r} is not a node id")
        out = (C.c_uint32 * n_bits)()
        self._eng._ck(self._lib.spf_graph_add_unpack(self._g, int(glwe_node), n_bits, out))
        return list(out)

    # ....pack(ctx, enc): one GLWE1 node = sum over i of X^i * nodes[i]
    def add_pack(self, nodes: Sequence[int]) -> int:
        nodes = list(nodes)
        n_bits = _check_n_bits("add_pack", len(nodes), self._eng.params.polynomial_degree)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= x < 1 << 32 for x in nodes):
            raise SpfError(1, "add_pack: the operands must be node ids")
        arr = (C.c_uint32 * n_bits)(*[int(x) for x in nodes])
        node = C.c_uint32()
        self._eng._ck(self._lib.spf_graph_add_pack(self._g, arr, n_bits, C.byref(node)))
        return node.value

    # blind_rotation (blind_rotation.rs:202-223): glwe_node * X^-(s << log_stride), s given by the GGSW1 nodes of its bits
    # (bit 0 first); one GLWE1 node per bit, returns the last
    def add_blind_rotation(self, glwe_node: int, shift_nodes: Sequence[int], log_stride: int = 0) -> int:
        nodes = list(shift_nodes)
        log_stride = _check_blind_rotation("add_blind_rotation", len(nodes), log_stride, self._eng.params.polynomial_degree)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= x < 1 << 32 for x in nodes + [glwe_node]):
            raise SpfError(1, "add_blind_rotation: the operands must be node ids")
        arr = (C.c_uint32 * len(nodes))(*[int(x) for x in nodes])
        node = C.c_uint32()
        self._eng._ck(self._lib.spf_graph_add_blind_rotation(self._g, int(glwe_node), arr, len(nodes), log_stride, C.byref(node)))
        return node.value

    # public_functional_keyswitch (public_functional_keyswitch.rs:74-148), message j to coefficient j: the LWE0 (or LWE1) nodes
    # -> one GLWE1 node
    def add_public_functional_keyswitch(self, nodes: Sequence[int]) -> int:
        nodes = list(nodes)
        lwe_count = _check_lwe_count("add_public_functional_keyswitch", len(nodes), self._eng.params.polynomial_degree)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= x < 1 << 32 for x in nodes):
            raise SpfError(1, "add_public_functional_keyswitch: the operands must be node ids")
        arr = (C.c_uint32 * lwe_count)(*[int(x) for x in nodes])
        node = C.c_uint32()
        self._eng._ck(self._lib.spf_graph_add_public_functional_keyswitch(self._g, arr, lwe_count, C.byref(node)))
        return node.value

    # the plaintext linear map of weight slot `slot` (Engine.load_lwe_linear_weights) over K LWE0 (or LWE1) nodes: M nodes of the
    # same kind, node m = sum over k of w[m][k] * nodes[k] (+ bias[m] on the body).  M=None asks the engine for the slot's shape;
    # the slot may also be loaded, and loaded again, after the graph is built (run() checks it)
    def add_lwe_linear(self, slot: int, nodes: Sequence[int], M=None) -> List[int]:
        nodes = list(nodes)
        if M is None:
            M = self._eng.lwe_linear_slot_shape(slot)[0]
        slot, M = _check_lwe_linear("add_lwe_linear", slot, len(nodes), M)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= x < 1 << 32 for x in nodes):
            raise SpfError(1, "add_lwe_linear: the operands must be node ids")
        arr = (C.c_uint32 * len(nodes))(*[int(x) for x in nodes])
        out = (C.c_uint32 * M)()
        self._eng._ck(self._lib.spf_graph_add_lwe_linear(self._g, slot, arr, len(nodes), M, out))
        return list(out)

    # the plaintext polynomial linear map of polynomial weight slot `slot` (Engine.load_glwe_poly_weights) over K GLWE1 nodes: M
    # GLWE1 nodes, node m = sum over k of w[m][k] * nodes[k] in Z_2^64[X]/(X^N + 1) (+ bias[m] on the body).  M=None asks the
    # engine for the slot's shape; the slot may also be loaded, and loaded again, after the graph is built (run() checks it)
    def add_glwe_poly_linear(self, slot: int, nodes: Sequence[int], M=None) -> List[int]:
        nodes = list(nodes)
        if M is None:
            M = self._eng.glwe_poly_slot_shape(slot)[0]
        slot, M = _check_lwe_linear("add_glwe_poly_linear", slot, len(nodes), M, GLWE_POLY_SLOTS, GLWE_POLY_MAX_ROWS)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= x < 1 << 32 for x in nodes):
            raise SpfError(1, "add_glwe_poly_linear: the operands must be node ids")
        arr = (C.c_uint32 * len(nodes))(*[int(x) for x in nodes])
        out = (C.c_uint32 * M)()
        self._eng._ck(self._lib.spf_graph_add_glwe_poly_linear(self._g, slot, arr, len(nodes), M, out))
        return list(out)

    def _add_glwe_ks(self, what: str, op: int, param, glwe_node) -> int:
        param = _check_glwe_ks(what, op, param, self._eng.params.polynomial_degree)
        if isinstance(glwe_node, bool) or not isinstance(glwe_node, (int, np.integer)) or not 0 <= glwe_node < 1 << 32:
            raise SpfError(1, f"{what}: {glwe_node!r} is not a node id")
        node = C.c_uint32()
        if op == GLWE_KEYSWITCH_NODE:
            st = self._lib.spf_graph_add_glwe_keyswitch(self._g, param, int(glwe_node), C.byref(node))
        elif op == GLWE_AUTOMORPHISM_NODE:
            st = self._lib.spf_graph_add_glwe_automorphism(self._g, param, int(glwe_node), C.byref(node))
        else:
            st = self._lib.spf_graph_add_glwe_trace(self._g, int(glwe_node), C.byref(node))
        self._eng._ck(st)
        return node.value

    # keyswitch_glwe_to_glwe (fft_ops.rs:457-495) of one GLWE1 node under the key of slot `slot` (Engine.load_glwe_keyswitch_key):
    # one GLWE1 node.  The slot may be loaded, and loaded again, after the graph is built (run() checks it)
    def add_glwe_keyswitch(self, slot: int, glwe_node: int) -> int:
        return self._add_glwe_ks("add_glwe_keyswitch", GLWE_KEYSWITCH_NODE, slot, glwe_node)

    # one round (1 .. log2 N) of the trace's loop (ops/automorphisms/mod.rs:72-83) under the context's automorphism key
    def add_glwe_automorphism(self, round: int, glwe_node: int) -> int:
        return self._add_glwe_ks("add_glwe_automorphism", GLWE_AUTOMORPHISM_NODE, round, glwe_node)

    # trace (ops/automorphisms/mod.rs:53-85) of one GLWE1 node
    def add_glwe_trace(self, glwe_node: int) -> int:
        return self._add_glwe_ks("add_glwe_trace", GLWE_TRACE_NODE, 0, glwe_node)

    # FheOp::Output* — returns the array run() fills
    def add_output(self, node: int, kind: ValueKind) -> np.ndarray:
        dtype = np.complex128 if ValueKind(kind) == ValueKind.GGSW1 else np.uint64
        out = np.zeros(self._words(kind) * 8 // np.dtype(dtype).itemsize, dtype=dtype)
        self._keep.append(out)
        self._eng._ck(self._lib.spf_graph_add_output(self._g, node, _ptr(out)))
        return out

    # CircuitProcessor::run_graph_blocking
    def run(self):
        self._eng._ck(self._lib.spf_graph_run(self._g))

    def member(self) -> int:
        """the member of the group the graph last ran on (0 for a graph of one engine)"""
        return int(self._lib.spf_graph_member(self._g))

    def stats(self):
        n, lv, la = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._eng._ck(self._lib.spf_graph_stats(self._g, C.byref(n), C.byref(lv), C.byref(la)))
        return {"nodes": n.value, "levels": lv.value, "launches": la.value}


class RecordedCircuit:
    """The builder calls of :class:`FheCircuit` kept as plain arrays, not bound to an executor: the same DAG can then be
    lowered into a gate graph (`lower`) or walked node by node the way the reference's `CircuitProcessor` does
    (circuit_processor/mod.rs:130-253) — `arrays()` is what such a per-operation driver takes."""

    _OUT_KIND = {FheOp.SampleExtract: ValueKind.LWE1, FheOp.KeyswitchL1toL0: ValueKind.LWE0, FheOp.Not: ValueKind.GLWE1,
                 FheOp.GlweAdd: ValueKind.GLWE1, FheOp.CMux: ValueKind.GLWE1, FheOp.GlevCMux: ValueKind.GLEV1,
                 FheOp.MultiplyGgswGlwe: ValueKind.GLWE1, FheOp.CircuitBootstrap: ValueKind.GGSW1,
                 FheOp.SchemeSwitch: ValueKind.GGSW1, FheOp.MulXN: ValueKind.GLWE1,
                 TableOp.PBS_UNIVARIATE: ValueKind.LWE1, TableOp.PBS_BIVARIATE: ValueKind.LWE1}

    def __init__(self, polynomial_degree: int = 2048):
        self.polynomial_degree = polynomial_degree   # bound of n_bits (add_unpack / add_pack); lower() checks the rest
        self.op: List[int] = []        # FheOp, NODE_UNPACK / NODE_PACK / NODE_ROT_CMUX / NODE_PUFKS / NODE_LWE_LINEAR / GLWE_POLY_LINEAR_NODE / GLWE_KEYSWITCH_NODE .. GLWE_TRACE_NODE, -1 input, -2 trivial constant
        self.kind: List[int] = []
        self.param: List[int] = []     # SampleExtract index / MulXN amount / trivial bit / unpack: bit index / pack: n_bits / GLWE keyswitch: slot / automorphism: round
        self.inputs: List[tuple] = []  # (pack nodes: all n_bits operands; public functional keyswitch nodes: all lwe_count)
        self.host: List = []           # inputs: the caller's array
        self.outputs: List[int] = []   # nodes, in add_output order
        self._unpack_width: dict = {}  # unpack node -> n_bits of its add_unpack call
        self._linear: dict = {}        # linear node -> (slot, M) of its add_lwe_linear / add_glwe_poly_linear call

    def _add(self, op, kind, param, inputs, host=None) -> int:
        self.op.append(int(op)); self.kind.append(int(kind)); self.param.append(int(param))
        self.inputs.append(tuple(int(i) for i in inputs)); self.host.append(host)
        return len(self.op) - 1

    def add_input(self, kind: ValueKind, value: np.ndarray) -> int:
        return self._add(-1, kind, 0, (), np.ascontiguousarray(value))

    def add_trivial(self, kind: ValueKind, bit: int) -> int:
        return self._add(-2, kind, bit, ())

    def add_op(self, op: FheOp, inputs: Sequence[int], param: int = 0) -> int:
        if any(i >= len(self.op) for i in inputs):
            raise SpfError(1, "operand is not a node of this circuit")
        node = _GLWE_KS_NODE_OF.get(int(op))
        if node is not None:   # recorded as the node of its named constructor, as spf_graph_add_op records it
            if len(inputs) != 1:   # (the library's text: over another count the value names no operation of spf_graph_add_op)
                raise SpfError(1, f"graph op: unknown operation: value {int(op)} over {len(inputs)} operands (the GLWE keyswitch, "
                                  "automorphism round and trace take one GLWE1)")
            return self._add_glwe_ks(_GLWE_KS_NAME[node], node, param, inputs[0])
        want = _PBS_IN_KINDS.get(int(op))
        if want is not None:   # the bootstraps by table: refused here as spf_graph_add_op refuses them
            if len(inputs) != len(want):
                raise SpfError(1, "graph op: wrong number of operands")
            inputs = [_check_node(graph_op(op).name, x, len(self.op)) for x in inputs]
            if any(self.kind[x] != k for x, k in zip(inputs, want)):
                raise SpfError(1, "graph op: operand has the wrong ciphertext type")
            if graph_op(op) == TableOp.PBS_UNIVARIATE:
                param = 0
            elif isinstance(param, bool) or not isinstance(param, (int, np.integer)) or not 0 <= param < 64:
                raise SpfError(1, "graph op: plaintext_bits must be below 64")
        return self._add(graph_op(op), self._OUT_KIND[graph_op(op)], param, inputs)

    def add_unpack(self, glwe_node: int, n_bits: int) -> List[int]:
        n_bits = _check_n_bits("add_unpack", n_bits, self.polynomial_degree)
        glwe_node = _check_node("add_unpack", glwe_node, len(self.op))
        if self.kind[glwe_node] != int(ValueKind.GLWE1):
            raise SpfError(1, "add_unpack: the operand is not an L1 GLWE")
        out = [self._add(NODE_UNPACK, ValueKind.LWE1, i, (glwe_node,)) for i in range(n_bits)]
        for n in out:
            self._unpack_width[n] = n_bits
        return out

    def add_pack(self, nodes: Sequence[int]) -> int:
        nodes = list(nodes)
        _check_n_bits("add_pack", len(nodes), self.polynomial_degree)
        nodes = [_check_node("add_pack", x, len(self.op)) for x in nodes]
        if any(self.kind[x] != int(ValueKind.GLWE1) for x in nodes):
            raise SpfError(1, "add_pack: an operand is not an L1 GLWE")
        return self._add(NODE_PACK, ValueKind.GLWE1, len(nodes), nodes)

    def add_blind_rotation(self, glwe_node: int, shift_nodes: Sequence[int], log_stride: int = 0) -> int:
        nodes = list(shift_nodes)
        log_stride = _check_blind_rotation("add_blind_rotation", len(nodes), log_stride, self.polynomial_degree)
        acc = _check_node("add_blind_rotation", glwe_node, len(self.op))
        nodes = [_check_node("add_blind_rotation", x, len(self.op)) for x in nodes]
        if self.kind[acc] != int(ValueKind.GLWE1):
            raise SpfError(1, "add_blind_rotation: the operand is not an L1 GLWE")
        if any(self.kind[x] != int(ValueKind.GGSW1) for x in nodes):
            raise SpfError(1, "add_blind_rotation: a selector is not an L1 GGSW")
        for i, sel in enumerate(nodes):   # acc' = cmux(sel, acc, X^-(2^(i + log_stride)) * acc)
            acc = self._add(NODE_ROT_CMUX, ValueKind.GLWE1, 1 << (i + log_stride), (sel, acc))
        return acc

    def add_public_functional_keyswitch(self, nodes: Sequence[int]) -> int:
        nodes = list(nodes)
        _check_lwe_count("add_public_functional_keyswitch", len(nodes), self.polynomial_degree)
        nodes = [_check_node("add_public_functional_keyswitch", x, len(self.op)) for x in nodes]
        if any(self.kind[x] not in (int(ValueKind.LWE0), int(ValueKind.LWE1)) for x in nodes):
            raise SpfError(1, "add_public_functional_keyswitch: an operand is not an LWE")
        if any(self.kind[x] != self.kind[nodes[0]] for x in nodes):
            raise SpfError(1, "add_public_functional_keyswitch: lwe0 and lwe1 operands mixed")
        return self._add(NODE_PUFKS, ValueKind.GLWE1, len(nodes), nodes)

    def add_lwe_linear(self, slot: int, nodes: Sequence[int], M: int) -> List[int]:
        """M is required here: a recording is bound to no engine that could be asked for the slot's shape"""
        nodes = list(nodes)
        slot, M = _check_lwe_linear("add_lwe_linear", slot, len(nodes), M)
        nodes = [_check_node("add_lwe_linear", x, len(self.op)) for x in nodes]
        if any(self.kind[x] not in (int(ValueKind.LWE0), int(ValueKind.LWE1)) for x in nodes):
            raise SpfError(1, "add_lwe_linear: an operand is not an LWE")
        if any(self.kind[x] != self.kind[nodes[0]] for x in nodes):
            raise SpfError(1, "add_lwe_linear: lwe0 and lwe1 operands mixed")
        out = [self._add(NODE_LWE_LINEAR, self.kind[nodes[0]], m, nodes) for m in range(M)]
        for n in out:
            self._linear[n] = (slot, M)
        return out

    def add_glwe_poly_linear(self, slot: int, nodes: Sequence[int], M: int) -> List[int]:
        """M is required here: a recording is bound to no engine that could be asked for the slot's shape"""
        nodes = list(nodes)
        slot, M = _check_lwe_linear("add_glwe_poly_linear", slot, len(nodes), M, GLWE_POLY_SLOTS, GLWE_POLY_MAX_ROWS)
        nodes = [_check_node("add_glwe_poly_linear", x, len(self.op)) for x in nodes]
        if any(self.kind[x] != int(ValueKind.GLWE1) for x in nodes):
            raise SpfError(1, "add_glwe_poly_linear: an operand is not an L1 GLWE")
        out = [self._add(GLWE_POLY_LINEAR_NODE, ValueKind.GLWE1, m, nodes) for m in range(M)]
        for n in out:
            self._linear[n] = (slot, M)
        return out

    def _add_glwe_ks(self, what: str, op: int, param, glwe_node) -> int:
        param = _check_glwe_ks(what, op, param, self.polynomial_degree)
        glwe_node = _check_node(what, glwe_node, len(self.op))
        if self.kind[glwe_node] != int(ValueKind.GLWE1):
            raise SpfError(1, f"{what}: the operand is not an L1 GLWE")
        return self._add(op, ValueKind.GLWE1, param, (glwe_node,))

    def add_glwe_keyswitch(self, slot: int, glwe_node: int) -> int:
        return self._add_glwe_ks("add_glwe_keyswitch", GLWE_KEYSWITCH_NODE, slot, glwe_node)

    def add_glwe_automorphism(self, round: int, glwe_node: int) -> int:
        return self._add_glwe_ks("add_glwe_automorphism", GLWE_AUTOMORPHISM_NODE, round, glwe_node)

    def add_glwe_trace(self, glwe_node: int) -> int:
        return self._add_glwe_ks("add_glwe_trace", GLWE_TRACE_NODE, 0, glwe_node)

    def linear_of(self, node: int) -> tuple:
        """(slot, M) of the add_lwe_linear or add_glwe_poly_linear call that made this linear node (its row index is `param[node]`)"""
        return self._linear[node]

    def add_output(self, node: int, kind: ValueKind) -> int:
        if self.kind[node] != int(kind):
            raise SpfError(1, "output kind does not match the node")
        self.outputs.append(int(node))
        return len(self.outputs) - 1

    def lower(self, engine: Engine):
        """-> (FheCircuit, [output arrays]) with the same nodes in the same order"""
        g = FheCircuit(engine)
        i = 0
        while i < len(self.op):
            if self.op[i] == NODE_UNPACK:    # the bit nodes of one add_unpack call are consecutive
                n_bits = self._unpack_width[i]
                bits = g.add_unpack(self.inputs[i][0], n_bits)
                assert bits == list(range(i, i + n_bits))
                i += n_bits
                continue
            if self.op[i] in _LINEAR_NODES:   # the row nodes of one add_lwe_linear / add_glwe_poly_linear call are consecutive
                slot, M = self._linear[i]
                rows = (g.add_lwe_linear if self.op[i] == NODE_LWE_LINEAR else g.add_glwe_poly_linear)(slot, self.inputs[i], M)
                assert rows == list(range(i, i + M))
                i += M
                continue
            if self.op[i] == NODE_PACK:
                n = g.add_pack(self.inputs[i])
            elif self.op[i] == NODE_PUFKS:
                n = g.add_public_functional_keyswitch(self.inputs[i])
            elif self.op[i] in _GLWE_KS_NODES:
                n = g._add_glwe_ks("lower", self.op[i], self.param[i], self.inputs[i][0])
            elif self.op[i] == NODE_ROT_CMUX:  # one step = a one-bit rotation whose stride is the step's rotation
                n = g.add_blind_rotation(self.inputs[i][1], [self.inputs[i][0]], self.param[i].bit_length() - 1)
            elif self.op[i] == -1:
                n = g.add_input(ValueKind(self.kind[i]), self.host[i])
            elif self.op[i] == -2:
                n = g.add_trivial(ValueKind(self.kind[i]), self.param[i])
            else:
                n = g.add_op(graph_op(self.op[i]), self.inputs[i], self.param[i])
            assert n == i
            i += 1
        return g, [g.add_output(n, ValueKind(self.kind[n])) for n in self.outputs]

    def arrays(self) -> dict:
        n = len(self.op)
        cached = getattr(self, "_arrays", None)
        if cached is not None and cached[0] == (n, len(self.outputs)):
            return cached[1]
        out = self._build_arrays()
        self._arrays = ((n, len(self.outputs)), out)
        return out

    def _build_arrays(self) -> dict:
        n = len(self.op)
        # a pack node's operands do not fit the three columns: they are ext[ext_at[i] : ext_at[i] + n_bits[i]] and its n_in is 0
        # (the executor's own layout, spf_graph.hpp); a public functional keyswitch node's lwe_count operands lie the same way.
        # n_bits is the integer's width on unpack and pack nodes, lwe_count on those, 0 elsewhere;
        # an unpack node's param is its bit index.  The M nodes of one add_lwe_linear call share ONE list of K operands
        # (n_bits = K, the same ext_at, param = the row index m); their weight slot and M are lin_slot / lin_rows, 0 elsewhere;
        # the M nodes of one add_glwe_poly_linear call lie the same way.
        ins = np.zeros((n, 3), dtype=np.uint32)
        n_in = np.zeros(n, dtype=np.uint32)
        n_bits = np.zeros(n, dtype=np.uint32)
        ext_at = np.zeros(n, dtype=np.uint32)
        lin_slot = np.zeros(n, dtype=np.uint32)
        lin_rows = np.zeros(n, dtype=np.uint32)
        ext: List[int] = []
        for i, t in enumerate(self.inputs):
            if self.op[i] in _LINEAR_NODES:
                lin_slot[i], lin_rows[i] = self._linear[i]
                n_bits[i] = len(t)
                if self.param[i] == 0:
                    ext_at[i] = len(ext)
                    ext.extend(t)
                else:
                    ext_at[i] = ext_at[i - 1]
                continue
            if self.op[i] in (NODE_PACK, NODE_PUFKS):
                n_bits[i], ext_at[i] = len(t), len(ext)
                ext.extend(t)
                continue
            if self.op[i] == NODE_UNPACK:
                n_bits[i] = self._unpack_width[i]
            ins[i, :len(t)] = t
            n_in[i] = len(t)
        keep = np.zeros(n, dtype=np.uint8)
        keep[self.outputs] = 1
        return {"op": np.array([o if o >= 0 else -1 for o in self.op], dtype=np.int32), "in": ins, "n_in": n_in,
                "param": np.array(self.param, dtype=np.uint64), "keep": keep,
                "n_bits": n_bits, "ext_at": ext_at, "ext": np.array(ext, dtype=np.uint32),
                "lin_slot": lin_slot, "lin_rows": lin_rows}

    @classmethod
    def from_arrays(cls, a: dict, kind: Sequence[int], host: Sequence, polynomial_degree: int = 2048) -> "RecordedCircuit":
        """the circuit that `arrays()` describes.  arrays() folds inputs and constants into op -1 (a per-operation driver is
        handed their values), so `kind` and `host` per node come with it, as in `self.kind` / `self.host`: a node with a host
        array is an input, one without a constant.  Outputs come back in node order."""
        g = cls(polynomial_degree)
        i, n = 0, len(a["op"])
        while i < n:
            op = int(a["op"][i])
            if op == NODE_UNPACK:
                w = int(a["n_bits"][i])
                g.add_unpack(int(a["in"][i, 0]), w)
                i += w
                continue
            if op in _LINEAR_NODES:
                at, rows = int(a["ext_at"][i]), int(a["lin_rows"][i])
                (g.add_lwe_linear if op == NODE_LWE_LINEAR else g.add_glwe_poly_linear)(int(a["lin_slot"][i]), [int(x) for x in a["ext"][at:at + int(a["n_bits"][i])]], rows)
                i += rows
                continue
            if op == NODE_PACK:
                at = int(a["ext_at"][i])
                g.add_pack([int(x) for x in a["ext"][at:at + int(a["n_bits"][i])]])
            elif op == NODE_PUFKS:
                at = int(a["ext_at"][i])
                g.add_public_functional_keyswitch([int(x) for x in a["ext"][at:at + int(a["n_bits"][i])]])
            elif op == NODE_ROT_CMUX:
                g.add_blind_rotation(int(a["in"][i, 1]), [int(a["in"][i, 0])], int(a["param"][i]).bit_length() - 1)
            elif op in _GLWE_KS_NODES:
                g._add_glwe_ks("from_arrays", op, int(a["param"][i]), int(a["in"][i, 0]))
            elif op == -1 and host[i] is not None:
                g.add_input(ValueKind(kind[i]), host[i])
            elif op == -1:
                g.add_trivial(ValueKind(kind[i]), int(a["param"][i]))
            else:
                g.add_op(graph_op(op), [int(x) for x in a["in"][i, :int(a["n_in"][i])]], int(a["param"][i]))
            i += 1
        for node in np.flatnonzero(a["keep"]):
            g.add_output(int(node), ValueKind(g.kind[int(node)]))
        return g
