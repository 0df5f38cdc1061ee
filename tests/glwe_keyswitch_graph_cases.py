"""Contexts, graphs and expected words shared by the tests of the GLWE keyswitch, automorphism and trace nodes of the gate graphs
(`spf_graph_add_glwe_keyswitch` / `_automorphism` / `_trace`): tests/test_gpu_glwe_keyswitch_graph.py,
tests/test_gpu_glwe_keyswitch_graph_cpp.py and tests/test_glwe_keyswitch_graph_host.py.  Test infrastructure.

Expected words come from the oracle functions of tests/glwe_keyswitch_cases.py (`oracle_keyswitch`, `oracle_round`, `O.trace`),
applied to the operand nodes' own output words; the nodes around (CMUX, XOR, polynomial linear rows, sample extracts) from the
oracle and `poly_linear_ref`.  There is no tolerance here."""
import numpy as np

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from spf_amd.graph import GLWE_AUTOMORPHISM_NODE, GLWE_KEYSWITCH_NODE, GLWE_TRACE_NODE
from tests import glwe_keyswitch_cases as KC
from tests import glwe_poly_cases as GC
from tests.blind_rotation_graph_cases import random_selectors
from tests.util import random_lwe_batch, to_engine_params

U = np.uint64
GLWE = ValueKind.GLWE1
KS, AU, TR = GLWE_KEYSWITCH_NODE, GLWE_AUTOMORPHISM_NODE, GLWE_TRACE_NODE
INVALID, NO_KEY = 1, 3
TUNED = "default128_6x7"
SHAPES = list(KC.SHAPES)
IN_PLACE = {True: "glwe_ks_kernel", False: "generic_glwe_ks_kernel"}
ROWS = {True: "glwe_ks_rows_kernel", False: "generic_glwe_ks_rows_kernel"}
# keyswitch-key slots: sk_a -> sk_b at the trace radix, another such key (other masks), the OTHER_RADIX key (the generic kernel on the
# tuned context), one that the fixtures never load
A2B_SLOT, SECOND_SLOT, OTHER_SLOT, EMPTY_SLOT = 3, 5, 9, 12
# polynomial weight slots: the 1 x 1 matrix X^-SHIFT, and a 1 x 1 matrix of two terms
SHIFT = 5
XINV_SLOT, TWO_TERM_SLOT = 33, 34
# (B of a group): four GLWEs share a workgroup of the tuned kernel — one unit with three padding units, a full workgroup, a ragged
# workgroup past the first; one workgroup per GLWE in the generic kernel
BATCHES = {TUNED: (1, 4, 5), "N256k3_7x5": (1, 3), "N16": (1, 3)}


def engine_params(P):
    return to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count, ss_radix_log=P.ss_radix_log,
                                       ss_radix_count=P.ss_count)


def xinv(N):
    """X^-SHIFT = -X^(N - SHIFT) as a 1 x 1 polynomial matrix"""
    return GC.csr([[[(N - SHIFT, -1)]]], 1, 1)


def two_terms(N):
    return GC.csr([[[(1, 3), (N - 1, -2)]]], 1, 1)


def slot_keys(c) -> dict:
    """slot -> (key words, spectra, (radix_log, radix_count)) of every slot load_keys fills"""
    P = c.P
    radix = (P.tr_radix_log, P.tr_count)
    keys = {A2B_SLOT: (c.ksk, c.ksk_fft, radix), SECOND_SLOT: KC.second_key(c) + (radix,)}
    if c.name == TUNED:
        keys[OTHER_SLOT] = KC.other_radix_key(c) + (KC.OTHER_RADIX,)
    return keys


def load_keys(eng, c):
    """the automorphism key, the keyswitch-key slots and the two polynomial weight slots, on an engine or a group"""
    eng.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
    for slot, (words, _, (lg, cnt)) in slot_keys(c).items():
        eng.load_glwe_keyswitch_key_std(slot, words, lg, cnt)
    eng.load_glwe_poly_weights(XINV_SLOT, xinv(c.P.N), None, shape=(1, 1))
    eng.load_glwe_poly_weights(TWO_TERM_SLOT, two_terms(c.P.N), None, shape=(1, 1))


def make_engine(shape):
    c = KC.case(shape)
    eng = spf_amd.Engine(engine_params(c.P))
    load_keys(eng, c)
    return eng


def modes(c=None, slot=A2B_SLOT):
    """(name, node kind, parameter) of the three operations as the tests draw them"""
    return [("keyswitch", KS, slot), ("automorphism", AU, 2), ("trace", TR, 0)]


def is_tuned(c, kind, param) -> bool:
    """does the hand-written kernel serve this node on the case's context?"""
    return c.name == TUNED and not (kind == KS and param == OTHER_SLOT)


def add_node(g, kind, param, node):
    """the node constructor of `kind` on an FheCircuit, a RecordedCircuit or a GraphBuilder"""
    if kind == KS:
        return g.add_glwe_keyswitch(param, node)
    if kind == AU:
        return g.add_glwe_automorphism(param, node)
    return g.add_glwe_trace(node)


def oracle_trace(c, x) -> np.ndarray:
    P = c.P
    return O.trace(np.asarray(x, dtype=U).reshape(-1), c.ak_fft.reshape(-1), P).reshape(P.k + 1, P.N)


def oracle_node(c, kind, param, x, keys=None) -> np.ndarray:
    """what a node of `kind` makes of the GLWE x (k+1, N): the oracle's words"""
    x = np.asarray(x, dtype=U).reshape(c.P.k + 1, c.P.N)
    if kind == KS:
        _, fft, radix = (keys or slot_keys(c))[param]
        return KC.oracle_keyswitch(c.P, x, fft, radix)
    if kind == AU:
        return KC.oracle_round(c, x, param)
    return oracle_trace(c, x)


def same_words(got, want) -> bool:
    got, want = np.asarray(got), np.asarray(want)
    return got.size == want.size and bool(np.array_equal(got.reshape(-1).view(U), want.reshape(-1).view(U)))


def glwe(c, words) -> np.ndarray:
    return np.asarray(words, dtype=U).reshape(c.P.k + 1, c.P.N)


def poly_row(c, triple, x) -> np.ndarray:
    """the one row of a 1 x 1 polynomial slot over the GLWE x"""
    P = c.P
    return GC.poly_linear_ref(glwe(c, x).reshape(1, 1, P.k + 1, P.N), triple, 1, 1)[0, 0]


def cmux(c, low, high, sel) -> np.ndarray:
    P = c.P
    return O.cmux(np.asarray(low).reshape(-1), np.asarray(high).reshape(-1), sel, P.N, P.k, P.cbs_radix_log, P.cbs_count)


# ---- the scattered graph ----------------------------------------------------------------------------------------------------------

class Scattered:
    """GLWE inputs interleaved with inputs of other kinds; on level 1 a CMUX, a polynomial linear row and two XORs, whose results lie
    in the blocks of three different groups.  With nodes: B nodes of one (kind, param) over the inputs [4, 0, 4, 2, 1][:B] (level
    1) and B over the level-1 results [poly row, CMUX, CMUX, XOR, XOR'][:B] (level 2), neither consecutive, each with one operand
    twice from B = 3 on.  Every node is an output."""
    INPUT_PICKS = [4, 0, 4, 2, 1]

    def __init__(self, eng, c, seed, kind=None, param=0, B=0):
        P = c.P
        self.c, self.kind, self.param, self.B = c, kind, param, B
        self.x = c.x
        self.sel = random_selectors(seed, 1, P)[0]
        lwes = random_lwe_batch(seed + 1, 2, P.k * P.N)
        g = self.g = spf_amd.FheCircuit(eng)
        ins = []
        for i, row in enumerate(self.x):            # GLWE | LWE1 | GLWE | GGSW | GLWE | LWE1 | GLWE | GLWE
            ins.append(g.add_input(GLWE, row))
            if i == 0 or i == 2:
                g.add_input(ValueKind.LWE1, lwes[i // 2])
            if i == 1:
                s = g.add_input(ValueKind.GGSW1, self.sel)
        cm = g.add_op(FheOp.CMux, [s, ins[0], ins[1]])
        pl = g.add_glwe_poly_linear(TWO_TERM_SLOT, [ins[2]], 1)[0]
        x1 = g.add_op(FheOp.GlweAdd, [ins[3], ins[4]])
        x2 = g.add_op(FheOp.GlweAdd, [ins[0], ins[4]])
        self.producers = [g.add_output(n, GLWE) for n in (pl, cm, x1, x2)]
        level1 = [pl, cm, cm, x1, x2][:B]
        self.over_inputs = [g.add_output(add_node(g, kind, param, ins[i]), GLWE) for i in self.INPUT_PICKS[:B]] if B else []
        self.over_level1 = [g.add_output(add_node(g, kind, param, n), GLWE) for n in level1] if B else []

    def producers_by_oracle(self):
        c, x, P = self.c, self.x, self.c.P
        return [poly_row(c, two_terms(P.N), x[2]), cmux(c, x[0], x[1], self.sel), O.glwe_xor(x[3].reshape(-1), x[4].reshape(-1), P.N, P.k),
                O.glwe_xor(x[0].reshape(-1), x[4].reshape(-1), P.N, P.k)]

    def check(self, what):
        """every output word: the producers by the oracle, the nodes by the oracle on their operands' own words"""
        c = self.c
        for j, (got, want) in enumerate(zip(self.producers, self.producers_by_oracle())):
            assert same_words(got, want), (what, "producer", j)
        for j, i in enumerate(self.INPUT_PICKS[:self.B]):
            assert same_words(self.over_inputs[j], oracle_node(c, self.kind, self.param, self.x[i])), (what, "over input", i)
        pl, cm, x1, x2 = self.producers
        for j, row in enumerate([pl, cm, cm, x1, x2][:self.B]):
            assert same_words(self.over_level1[j], oracle_node(c, self.kind, self.param, row)), (what, "over level 1", j)


# ---- reload: one graph, four runs, another key before the last ---------------------------------------------------------------------

def reload_rounds(eng, c, slot=7):
    """keyswitch nodes over scattered inputs feeding keyswitch nodes in place, run three times on new contents, then once more after
    the slot was loaded again with another key: every run gives the words of the key loaded when it ran.  With SPF_GRAPH_CAPTURE=1
    the second run captures and the third replays, so the reload falls after the capture."""
    P = c.P
    radix = (P.tr_radix_log, P.tr_count)
    first, second = (c.ksk, c.ksk_fft, radix), KC.second_key(c) + (radix,)
    eng.load_glwe_keyswitch_key_std(slot, first[0], *radix)
    bufs = [c.x[i].copy() for i in (3, 0, 3)]
    g = spf_amd.FheCircuit(eng)
    ins = [g.add_input(GLWE, b) for b in bufs]
    a = [g.add_glwe_keyswitch(slot, n) for n in (ins[2], ins[0], ins[1])]
    b = [g.add_glwe_keyswitch(slot, n) for n in a]
    outs = [g.add_output(n, GLWE) for n in a + b]

    def want(key):
        mid = [oracle_node(c, KS, slot, bufs[i], {slot: key}) for i in (2, 0, 1)]
        return mid + [oracle_node(c, KS, slot, m, {slot: key}) for m in mid]

    for run in range(4):
        key = first
        if run == 3:
            eng.load_glwe_keyswitch_key_std(slot, second[0], *radix)
            key = second
        for j, buf in enumerate(bufs):               # new contents at every run: a replay reads the inputs again
            buf[...] = c.x[(run + j) % KC.ITEMS]
        g.run()
        assert g.stats()["launches"] == 2, g.stats()
        for j, (got, w) in enumerate(zip(outs, want(key))):
            assert same_words(got, w), (c.name, "run", run, "node", j)
    assert not same_words(outs[0], oracle_node(c, KS, slot, bufs[2], {slot: first})), "the two keys give the same words: the case proves nothing"
    g.close()
