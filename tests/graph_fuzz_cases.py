"""The generator of the random differential tests of gate graphs (tests/test_graph_fuzz_host.py, tests/test_gpu_graph_fuzz.py):
`draw_circuit(seed, P, profile) -> (RecordedCircuit, facts)`, deterministic in its arguments, numpy only.

A circuit is a typed DAG over the five value kinds with every node kind of the executor in it: every operation of the table
(spf_ops.hpp) that has a `spf_graph_op` and the five constructors (unpack, pack, blind rotation, public functional keyswitch,
plaintext linear map, plaintext polynomial linear map, GLWE keyswitch / automorphism round / trace).  The weights of the linear
maps are no part of a circuit: `draw_linear_slots(linear_seed)` draws them for a fixed table of slot shapes, so that one engine
(or one group) loads them once for every circuit it runs; `draw_glwe_poly_slots` and `draw_glwe_ksk_slots` do the same for the
polynomial weights and the GLWE keyswitch keys.
The generator BUILDS the layouts in which the executor's plan takes another branch (PATTERNS below) and, for each, records the
claim that makes it one: which nodes have to share a group, lie in consecutive rows, or stand on different levels.  The claims
are checked against `circuit_model.planned_levels`, the executor's own level passes, so `facts` names a pattern only if the
circuit really holds it once the planner has moved the bootstraps and the conversion heads."""
import numpy as np

from spf_amd import FheOp, RecordedCircuit, TableOp, ValueKind
from spf_amd.graph import (GLWE_KSK_SLOTS, GLWE_POLY_SLOTS, NODE_GLWE_AUTOMORPHISM, NODE_GLWE_KEYSWITCH, NODE_GLWE_POLY_LINEAR,
                           NODE_GLWE_TRACE, NODE_LWE_LINEAR, NODE_PACK, NODE_PUFKS, NODE_ROT_CMUX, NODE_UNPACK)
from tests import glwe_poly_cases as GC
from tests.blind_rotation_graph_cases import random_selectors
from tests.circuit_model import kind_name, planned_levels
from tests.glwe_keyswitch_cases import OTHER_RADIX
from tests.lwe_linear_cases import class_weights

PROFILES = ("full", "pushable", "small")
CMUX_WIDTHS = (1, 2, 3, 5, 40, 70, 260, 300)           # test_gpu_fuzz.py's list: both CMUX kernels of the tuned context
_WIDTH_SETS = ((260, 2, 5), (40, 70, 3), (300, 1))      # by seed % 3: three consecutive seeds draw every width
MAX_NODES = 850                                         # "about 400", the ~165 nodes of LINEAR_PATTERNS (rows are nodes) and the
#                                                         ~225 of GLWE_PATTERNS (620 before the GLWE section)
MAX_NODES_SMALL = 76                                    # ... a 9-row and a 2-row layer with their user; a 5-row and a 1-row
#                                                         polynomial layer and a node of each keyswitch mode (66 before)
MAX_BOOTSTRAPS = 16                                     # of each of the three kinds

DEFAULT_CASES, DEFAULT_SEED = 3, 20260701               # of tests/test_gpu_graph_fuzz.py (SPF_FUZZ_CASES / SPF_FUZZ_SEED)
PUFKS_RADICES = ((4, 8), (4, 4), (5, 3))                # (log, count) on the tuned context: two hand-written, one generic


def case_seed(seed, test, case) -> int:
    """the circuit seed of case `case` of test number `test` of the GPU file (0 lowered, 1 pushed, 2 group jobs, 3 parameter sets)"""
    return seed + 1000 * test + case


def tuned_pufks_kind(case):
    """the tuned context's operand kind: LWE0 in all cases but one in nine (an LWE1 key is 268 MB, a second per node on the oracle)"""
    return ValueKind.LWE1 if case % 9 == 1 else ValueKind.LWE0


L0, L1, GL, GG, GV = ValueKind.LWE0, ValueKind.LWE1, ValueKind.GLWE1, ValueKind.GGSW1, ValueKind.GLEV1

PUFKS_PATTERNS = (
    "pufks_rows_consecutive", "pufks_rows_scattered_with_repeats", "pufks_count_1", "pufks_count_2", "pufks_count_large",
    "pufks_two_of_one_count_on_one_level", "pufks_result_as_table", "pufks_result_as_cmux_operand",
    "pufks_result_as_unpack_source", "unpack_source_is_a_keyswitch_node")
PATTERNS = tuple(f"cmux_width_{w}" for w in CMUX_WIDTHS) + (
    "pbs_group_one_table", "pbs_group_tables_out_of_order", "pbs_table_computed_later_than_its_lwes",
    "pbs_univariate_and_bivariate_on_one_level", "bivariate_both_inputs_consecutive", "bivariate_one_input_scattered",
    "bivariate_same_node_twice", "bivariate_plaintext_bits_0", "bivariate_plaintext_bits_middle", "bivariate_plaintext_bits_63",
    "slack_circuit_bootstrap_early_next_to_late", "slack_univariate_early_next_to_late", "slack_bivariate_early_next_to_late",
    "sample_extract_users_on_two_levels", "keyswitch_users_on_two_levels", "sample_extract_is_also_an_output",
    "keyswitch_is_also_an_output",
    "unpack_two_calls_consecutive_sources", "unpack_two_calls_scattered_sources", "unpack_two_widths_on_one_level",
    "unpack_source_is_a_pack",
    "pack_operands_from_two_levels", "pack_operand_repeated", "pack_two_of_one_width_on_one_level", "pack_width_1",
    "pack_width_2", "pack_width_above_8",
    "rotation_bits_1", "rotation_bits_2", "rotation_bits_3", "rotation_bits_4", "rotation_log_stride_0",
    "rotation_log_stride_larger", "rotation_chains_share_selectors", "rotation_chains_distinct_selectors",
    "rotation_two_rotations_on_one_level", "rotation_selector_input", "rotation_selector_trivial",
    "rotation_selector_circuit_bootstrap", "rotation_selector_scheme_switch_of_glev_cmux", "rotation_middle_step_used_elsewhere",
    "cmux_glev_cmux_and_multiply_share_a_selector_on_one_level",
    "output_of_every_kind", "output_given_twice", "outputs_every_node_of_the_last_level",
    "trivial_of_every_kind_both_bits") + PUFKS_PATTERNS

# the layouts of the plaintext linear map (spf_graph_add_lwe_linear).  "in place": ALL operand rows of the layer's group are
# successive members of one group, in the group's layer-major order; "scattered": the claim rests on a repeated operand or on a
# pair of neighbours that lie in descending order in the arena, which no arena layout makes consecutive (`_View.scattered`)
LINEAR_PATTERNS = (
    "linear_in_place_over_a_keyswitch_group", "linear_in_place_over_a_univariate_group", "linear_in_place_over_unpack_bits",
    "linear_in_place_over_a_previous_layer", "linear_two_layers_in_place",
    "linear_scattered_previous_layer_permuted", "linear_scattered_operand_repeated", "linear_scattered_three_levels_inputs_and_constants",
    "linear_two_layers_one_consecutive_one_scattered", "linear_two_layers_over_one_operand_list",
    "linear_two_slots_of_one_shape_on_one_level", "linear_both_operand_kinds_on_one_level_with_one_slot", "linear_shape_1_1",
    "linear_pulls_a_keyswitch_up", "linear_pulls_a_sample_extract_up", "linear_follows_a_moved_table_bootstrap",
    "linear_row_into_a_circuit_bootstrap", "linear_row_into_a_univariate_bootstrap", "linear_rows_into_a_bivariate_consecutive",
    "linear_row_into_a_bivariate_scattered", "linear_rows_into_a_keyswitch", "linear_rows_into_a_functional_keyswitch_in_order",
    "linear_rows_into_a_functional_keyswitch_with_a_repeat", "linear_row_is_an_output_and_has_users", "linear_layer_partly_used",
    "linear_last_group_in_place_with_one_limb_weights")
PATTERNS += LINEAR_PATTERNS

# ---- the weight slots: (slot, M, K, class of lwe_linear_cases.class_weights, bias).  M below, at and above LWE_LINEAR_VT = 8
# (1, 2 .. 5, 8, 9, 17), K = 1 and off and on the unroll factor 4; slots 0 and 1 have one shape; every class; bias and none; the
# slot ids run to the last one (SPF_LWE_LINEAR_SLOTS - 1)
S_A, S_B, S_WIDE, S_PERM, S_REPEAT, S_MIXED, S_PAIR, S_ONE, S_SMALL, S_BITS, S_LAST, S_TWICE = 0, 1, 2, 3, 7, 12, 21, 33, 40, 47, 62, 63
LINEAR_SLOTS = (
    (S_A, 8, 4, 2, True), (S_B, 8, 4, "beyond", False), (S_WIDE, 17, 3, 2, True), (S_PERM, 3, 8, "int64", True),
    (S_REPEAT, 9, 5, 3, False), (S_MIXED, 1, 7, "beyond", True), (S_PAIR, 3, 2, "int64", False), (S_ONE, 1, 1, 1, True),
    (S_SMALL, 2, 9, 2, False), (S_BITS, 5, 3, 3, False), (S_LAST, 9, 5, 1, True), (S_TWICE, 2, 2, 1, False))
LINEAR_SHAPE = {slot: (M, K) for slot, M, K, _, _ in LINEAR_SLOTS}
LINEAR_CLASS = {slot: cls for slot, _, _, cls, _ in LINEAR_SLOTS}


def draw_linear_slots(linear_seed) -> dict:
    """{slot: (weights int64 (M, K), bias uint64 (M,) or None)} for the table LINEAR_SLOTS: the shapes, the classes and which slots
    have a bias are fixed, the contents are drawn from `linear_seed`"""
    out = {}
    for slot, M, K, cls, bias in LINEAR_SLOTS:
        w = class_weights(64 * int(linear_seed) + slot, M, K, cls)
        b = np.random.default_rng([0x6A7, int(linear_seed), slot]).integers(0, 1 << 64, M, dtype=np.uint64) if bias else None
        out[slot] = (w, b)
    return out


# ---- the plaintext polynomial linear map (spf_graph_add_glwe_poly_linear) and the GLWE keyswitch, automorphism round and trace
# (spf_graph_add_glwe_keyswitch / _automorphism / _trace).  "in place" and "scattered" as above: in place is claimed for ALL operand
# rows of the node's whole group (`_View.in_place`), scattered rests on a repeat or a descending pair (`_View.scattered`)
GLWE_KS_KINDS = (NODE_GLWE_KEYSWITCH, NODE_GLWE_AUTOMORPHISM, NODE_GLWE_TRACE)
GLWE_MODES = (("keyswitch", NODE_GLWE_KEYSWITCH), ("automorphism", NODE_GLWE_AUTOMORPHISM), ("trace", NODE_GLWE_TRACE))
_MODE_LAYOUTS = ("in_place_over_a_cmux_group", "in_place_over_a_pack_group", "in_place_over_a_polynomial_layer",
                 "in_place_over_rotation_chains", "in_place_over_its_own_mode", "scattered_with_a_repeat", "scattered_descending",
                 "group_of_1", "group_of_4", "group_of_5")
_MODE_LAYOUTS_WITH_POLY = ("in_place_over_a_polynomial_layer",)        # what a circuit without polynomial layers cannot hold
GLWE_KS_PATTERNS = tuple(f"glwe_{mode}_{layout}" for mode, _ in GLWE_MODES for layout in _MODE_LAYOUTS) + (
    "glwe_two_keyswitch_slots_on_one_level", "glwe_other_radix_slot_and_trace_radix_slot_on_one_level",
    "glwe_two_automorphism_rounds_on_one_level", "glwe_all_three_modes_over_one_operand_on_one_level",
    "glwe_automorphism_round_1", "glwe_automorphism_round_log2_n", "glwe_last_keyswitch_group_scattered",
    "glwe_result_as_unpack_source", "glwe_result_into_a_sample_extract_and_a_keyswitch", "glwe_result_as_pack_operand",
    "glwe_results_as_cmux_low_and_high", "glwe_result_as_rotation_accumulator", "glwe_result_as_univariate_table",
    "glwe_result_as_bivariate_table", "glwe_input_reaches_the_outputs_through_the_new_kinds_only")
GLWE_POLY_PATTERNS = (
    "poly_in_place_over_a_cmux_group", "poly_in_place_over_a_pack_group", "poly_in_place_over_a_previous_layer",
    "poly_in_place_over_a_keyswitch_group", "poly_two_layers_in_place", "poly_scattered_previous_layer_permuted",
    "poly_scattered_operand_repeated", "poly_scattered_three_levels_inputs_and_constants",
    "poly_two_layers_one_consecutive_one_scattered", "poly_two_slots_of_one_shape_on_one_level",
    "poly_constants_only_in_place", "poly_constants_only_scattered", "poly_general_in_place", "poly_general_scattered",
    "poly_empty_matrix_with_a_bias", "poly_shape_1_1", "poly_follows_a_cmux_on_a_moved_circuit_bootstrap", "poly_layer_partly_used",
    "poly_row_is_an_output_and_has_users", "poly_over_results_of_the_keyswitch_family", "poly_last_group_in_place_general",
    "glwe_sample_extract_users_on_two_levels", "glwe_pulls_a_sample_extract_up")
GLWE_PATTERNS = GLWE_KS_PATTERNS + GLWE_POLY_PATTERNS
PATTERNS += GLWE_PATTERNS
# what `pushable` holds of them: no polynomial layer (no submit by handle), so nothing that needs one, nor an LWE linear layer
GLWE_PUSHABLE_PATTERNS = tuple(n for n in GLWE_KS_PATTERNS if not n.endswith(_MODE_LAYOUTS_WITH_POLY))

# keyswitch-key slots: two at the context's trace radix, one at another radix (the generic kernel inside a tuned graph); ids 0 and last
K_A, K_OTHER, K_B = 0, 9, GLWE_KSK_SLOTS - 1
GLWE_KSK_TABLE = (K_A, K_OTHER, K_B)
# polynomial weight slots: (slot, M, K, class, bias).  M below, at and above GLWE_POLY_VT = 4, K on and off the stream kernel's
# unroll of 4 (glwe_poly_graph_cases.SCATTERED_SHAPES); P_A / P_B and P_ONE / P_UNIT and P_ROW / P_EMPTY are pairs of one shape
# (P_A is the last slot id: of the polynomial groups of a level, its groups are the last in key order, so the last to be launched)
P_EMPTY, P_B, P_ONE, P_UNIT, P_ROW, P_WIDE, P_TALL, P_A = 0, 1, 5, 17, 22, 40, 51, GLWE_POLY_SLOTS - 1
GLWE_POLY_TABLE = (
    (P_A, 4, 4, "general", True), (P_B, 4, 4, "constants", False), (P_ONE, 1, 1, "general", False), (P_UNIT, 1, 1, "constants", True),
    (P_ROW, 1, 5, "constants", False), (P_WIDE, 5, 7, "general", True), (P_TALL, 9, 2, "general", False), (P_EMPTY, 1, 5, "empty", True))
GLWE_POLY_SHAPE = {slot: (M, K) for slot, M, K, _, _ in GLWE_POLY_TABLE}
GLWE_POLY_CLASS = {slot: cls for slot, _, _, cls, _ in GLWE_POLY_TABLE}


def other_radix_of(P) -> tuple:
    """(radix_log, radix_count) of slot K_OTHER: glwe_keyswitch_cases.OTHER_RADIX on the tuned shape (the hand-written kernel
    serves the trace radix alone there), elsewhere any radix that is not the trace's"""
    if (P.N, P.k) == (2048, 1):
        return OTHER_RADIX
    return (4, 3) if (P.tr_radix_log, P.tr_count) != (4, 3) else (5, 2)


def draw_glwe_ksk_slots(key_seed, P, other_radix=None) -> dict:
    """{slot: (words uint64 (k, L, k+1, N), radix_log, radix_count)} for GLWE_KSK_TABLE: K_A and K_B at the context's trace radix
    with different words, K_OTHER at `other_radix` (`other_radix_of(P)` unless given).  Uniform words: parity needs no honest key
    (pbs_graph_cases.pufks_key).  Only the contents depend on `key_seed`"""
    trace = (P.tr_radix_log, P.tr_count)
    out = {}
    for slot, (lg, cnt) in ((K_A, trace), (K_OTHER, other_radix or other_radix_of(P)), (K_B, trace)):
        words = np.random.default_rng([0x6A9, int(key_seed), slot, P.N, P.k]).integers(0, 1 << 64, (P.k, cnt, P.k + 1, P.N), dtype=np.uint64)
        out[slot] = (words, int(lg), int(cnt))
    return out


def draw_glwe_poly_slots(poly_seed, N) -> dict:
    """{slot: (CSR triple, bias uint64 (M, N) or None, (M, K))} for GLWE_POLY_TABLE.  "general": exponents from
    glwe_poly_cases.seam_exponents(N), and polynomial (0, 0) holds every seam exponent and every EXTREME_COEFFICIENT;
    "constants": exponent 0 only (the stream kernels), the extreme coefficients planted likewise; "empty": no term at all.
    The shapes, the classes and which slots have a bias are fixed, the contents are drawn from `poly_seed`"""
    seams, cs = GC.seam_exponents(N), GC.EXTREME_COEFFICIENTS
    out = {}
    for slot, M, K, cls, bias in GLWE_POLY_TABLE:
        seed = 64 * int(poly_seed) + slot
        if cls == "empty":
            polys = [[[] for _ in range(K)] for _ in range(M)]
        else:
            polys = GC.random_polys(seed, M, K, N, terms=3 if cls == "general" else 2, cls="seams" if cls == "general" else "constants")
            exps = seams if cls == "general" else [0]
            polys[0][0] = polys[0][0][:1] + [(exps[i % len(exps)], cs[i % len(cs)]) for i in range(max(len(exps), len(cs)))]
        out[slot] = (GC.csr(polys, M, K), GC.random_bias(seed, M, N) if bias else None, (M, K))
    return out


def words_of(P, kind) -> int:
    return {L0: P.lwe_n + 1, L1: P.k * P.N + 1, GL: P.glwe_len, GG: 2 * P.cbs_ggsw_fft_len, GV: P.cbs_count * P.glwe_len}[ValueKind(kind)]


def random_value(rng, P, kind) -> np.ndarray:
    """uniform 64-bit words; GGSW: complex values at 2^58 (blind_rotation_graph_cases.random_selectors)"""
    if ValueKind(kind) == GG:
        return random_selectors(int(rng.integers(1 << 62)), 1, P)[0]
    return rng.integers(0, 1 << 64, size=words_of(P, kind), dtype=np.uint64)


def refill_inputs(rec, P, seed):
    """new random contents in the input arrays of `rec`, in place: the same graph on new data"""
    rng = np.random.default_rng([0x6A6, seed])
    for i, op in enumerate(rec.op):
        if op == -1:
            new = random_value(rng, P, rec.kind[i])
            rec.host[i].view(np.uint64).reshape(-1)[...] = new.view(np.uint64).reshape(-1)


def group_key(rec, levels, i):
    """(level, kind, parameter) in the order the planner keys its groups (spf_graph_plan.hpp's GroupKey has named fields; this
    packed number is the independent statement of their order: tests/test_graph_plan.py)"""
    op = rec.op[i]
    if op == NODE_UNPACK:
        return levels[i], op, rec._unpack_width[i]
    if op == NODE_PACK:
        return levels[i], op, len(rec.inputs[i])
    if op == NODE_PUFKS:
        return levels[i], op, len(rec.inputs[i]) | rec.kind[rec.inputs[i][0]] << 32
    if op == NODE_LWE_LINEAR:       # K | M << 32 | slot << 48 | kind << 56
        slot, rows = rec.linear_of(i)
        return levels[i], op, len(rec.inputs[i]) | rows << 32 | slot << 48 | rec.kind[i] << 56
    if op == NODE_GLWE_POLY_LINEAR:  # the same packing; the kind is GLWE1
        slot, rows = rec.linear_of(i)
        return levels[i], op, len(rec.inputs[i]) | rows << 32 | slot << 48 | int(GL) << 56
    return levels[i], op, rec.param[i]      # (GLWE keyswitch: the slot, automorphism: the round, trace: 0)


def groups_of(rec, levels) -> dict:
    """{group key: members in node order}: a group's results are consecutive rows in that order"""
    out = {}
    for i, op in enumerate(rec.op):
        if op >= 0:
            out.setdefault(group_key(rec, levels, i), []).append(i)
    return out


class _Builder:
    def __init__(self, seed, P, profile):
        self.P, self.profile = P, profile
        self.rng = np.random.default_rng([0x6A5, seed, P.N, P.k, P.lwe_n, PROFILES.index(profile)])
        # the GLWE section's own generator: what it draws leaves every draw of the sections before it as it was
        self.grng = np.random.default_rng([0x6A8, seed, P.N, P.k, P.lwe_n, PROFILES.index(profile)])
        self.rec = RecordedCircuit(P.N)
        self.pool = {k: [] for k in ValueKind}
        self.claims = []        # (name, f(view) -> bool)
        self.keep = []          # nodes that are outputs whatever the sample draws
        self.dead = set()       # nodes that nobody uses and that are no outputs either
        self.lvl = []

    # ---- nodes
    def _note(self, node):
        self.pool[ValueKind(self.rec.kind[node])].append(node)
        while len(self.lvl) <= node:    # as soon as possible: what plan() starts from
            i = len(self.lvl)
            self.lvl.append(1 + max((self.lvl[j] for j in self.rec.inputs[i]), default=0) if self.rec.op[i] >= 0 else 0)
        return node

    def older(self, kind, level):
        """the nodes of a kind that are ready by `level`"""
        return [i for i in self.pool[ValueKind(kind)] if self.lvl[i] <= level]

    def inp(self, kind):
        return self._note(self.rec.add_input(kind, random_value(self.rng, self.P, kind)))

    def triv(self, kind, bit):
        return self._note(self.rec.add_trivial(kind, bit))

    def op(self, op, ins, param=0):
        return self._note(self.rec.add_op(op, ins, param))

    def unpack(self, src, w):
        bits = self.rec.add_unpack(src, w)
        for b in bits:
            self._note(b)
        return bits

    def pack(self, nodes):
        return self._note(self.rec.add_pack(nodes))

    def pufks(self, nodes):
        return self._note(self.rec.add_public_functional_keyswitch(nodes))

    def linear(self, slot, nodes):
        """one layer of weight slot `slot` -> its M row nodes"""
        M, K = LINEAR_SHAPE[slot]
        assert len(nodes) == K, (slot, K, len(nodes))
        return [self._note(r) for r in self.rec.add_lwe_linear(slot, nodes, M)]

    def poly_linear(self, slot, nodes):
        """one polynomial layer of weight slot `slot` -> its M row nodes"""
        M, K = GLWE_POLY_SHAPE[slot]
        assert len(nodes) == K, (slot, K, len(nodes))
        return [self._note(r) for r in self.rec.add_glwe_poly_linear(slot, nodes, M)]

    def glwe_keyswitch(self, slot, node):
        return self._note(self.rec.add_glwe_keyswitch(slot, node))

    def glwe_automorphism(self, round, node):
        return self._note(self.rec.add_glwe_automorphism(round, node))

    def glwe_trace(self, node):
        return self._note(self.rec.add_glwe_trace(node))

    def glwe_node(self, kind, param, node):
        """a node of one of GLWE_KS_KINDS"""
        if kind == NODE_GLWE_KEYSWITCH:
            return self.glwe_keyswitch(param, node)
        return self.glwe_automorphism(param, node) if kind == NODE_GLWE_AUTOMORPHISM else self.glwe_trace(node)

    def ginp(self, kind):
        """an input whose contents come from the GLWE section's generator"""
        return self._note(self.rec.add_input(kind, random_value(self.grng, self.P, kind)))

    def rotation(self, acc, sels, log_stride=0):
        first = len(self.rec.op)
        last = self.rec.add_blind_rotation(acc, sels, log_stride)
        self._note(last)        # (the steps before it are drawn as operands only on purpose: most chains stay whole)
        return list(range(first, last + 1))

    def pick(self, kind, count=None, among=None):
        src = self.pool[ValueKind(kind)] if among is None else among
        at = self.rng.integers(0, len(src), size=1 if count is None else count)
        return src[int(at[0])] if count is None else [src[int(a)] for a in at]

    def index(self):
        return int(self.rng.integers(0, self.P.N))

    def claim(self, name, fn=None):
        self.claims.append((name, fn if fn is not None else (lambda v: True)))


class _View:
    """the finished circuit as the planner sees it: what the claims are checked against"""

    def __init__(self, rec):
        self.rec = rec
        self.level = planned_levels(rec)
        self.asap = [0] * len(rec.op)
        for i, op in enumerate(rec.op):
            if op >= 0:
                self.asap[i] = 1 + max((self.asap[j] for j in rec.inputs[i]), default=0)
        self.groups = groups_of(rec, self.level)
        self.users = [[] for _ in rec.op]
        for i, ins in enumerate(rec.inputs):
            for j in set(ins):
                self.users[j].append(i)

    def key(self, i):
        return group_key(self.rec, self.level, i)

    def one_group(self, nodes):
        return len({self.key(i) for i in nodes}) == 1

    def whole_group(self, nodes):
        """the nodes are a group, all of it"""
        return self.one_group(nodes) and sorted(self.groups[self.key(nodes[0])]) == sorted(nodes)

    def rows(self, nodes):
        """the rows lie consecutively in this order: successive members of one group"""
        if not self.one_group(nodes):
            return False
        members = self.groups[self.key(nodes[0])]
        at = [members.index(i) for i in nodes]
        return all(b == a + 1 for a, b in zip(at, at[1:]))

    def position(self, i):
        """orders the nodes as plan() lays them out in the arena: inputs and constants in node order, then the groups by (level,
        kind, parameter), a group's members in node order"""
        if self.rec.op[i] < 0:
            return 0, -3, 0, i
        return self.key(i) + (self.groups[self.key(i)].index(i),)

    def scattered(self, nodes):
        """a repeat, or two neighbours of which the second lies no later than the first: consecutive under no layout"""
        return any(self.position(b) <= self.position(a) for a, b in zip(nodes, nodes[1:]))

    def linear_operands(self, node):
        """the operand rows of the whole group of a linear or polynomial linear node, layer-major as plan() collects them; of a GLWE
        keyswitch, automorphism or trace node: one per member"""
        members = self.groups[self.key(node)]
        if self.rec.op[node] in GLWE_KS_KINDS:
            return [self.rec.inputs[m][0] for m in members]
        M = self.rec.linear_of(node)[1]
        return [j for q in range(0, len(members), M) for j in self.rec.inputs[members[q]]]

    def in_place(self, node):
        """the node's group (linear, polynomial linear, GLWE keyswitch family) reads its operands where they lie"""
        ops = self.linear_operands(node)
        return all(self.rec.op[j] >= 0 for j in ops) and self.rows(ops)

    def user_levels(self, i):
        return {self.level[u] for u in self.users[i]}

    def moved_next_to_late(self, early, late):
        """ready early and not needed for at least two levels, run on the level of one that is ready late"""
        return self.asap[early] + 2 <= self.level[early] == self.level[late] and self.asap[late] >= self.asap[early] + 2


def _sources(b, n_glwe, n_l1, n_l0, n_ggsw, n_glev, trivials=True):
    s = {GL: [b.inp(GL) for _ in range(n_glwe)], L1: [b.inp(L1) for _ in range(n_l1)], L0: [b.inp(L0) for _ in range(n_l0)],
         GG: [b.inp(GG) for _ in range(n_ggsw)], GV: [b.inp(GV) for _ in range(n_glev)]}
    t = {(k, bit): b.triv(k, bit) for k in (ValueKind if trivials else ()) for bit in (0, 1)}
    if trivials:
        b.claim("trivial_of_every_kind_both_bits", lambda v: {(b.rec.kind[i], b.rec.param[i]) for i, op in enumerate(b.rec.op) if op == -2}
                == {(int(k), bit) for k in ValueKind for bit in (0, 1)})
    return s, t


def _outputs(b, sample):
    """the kept nodes (one of them twice), every node of the last level, every node nobody uses, a random sample of the rest"""
    rec = b.rec
    v = _View(rec)
    top = max(v.level)
    last = [i for i, op in enumerate(rec.op) if op >= 0 and v.level[i] == top]
    assert not any(v.users[i] or v.level[i] == top for i in b.dead)
    unused = [i for i, op in enumerate(rec.op) if op >= 0 and not v.users[i] and i not in b.dead]
    rest = [i for i, op in enumerate(rec.op) if op >= 0 and i not in b.dead]
    drawn = [rest[int(a)] for a in b.rng.integers(0, len(rest), size=min(sample, len(rest)))]
    order, seen = [], set()
    for i in b.keep + last + unused + drawn:
        if i not in seen:
            seen.add(i)
            order.append(i)
    order.insert(len(order) // 2, order[0])                 # one node given as an output twice
    for i in order:
        rec.add_output(i, ValueKind(rec.kind[i]))
    b.claim("output_given_twice", lambda w: len(rec.outputs) > len(set(rec.outputs)))
    b.claim("output_of_every_kind", lambda w: {rec.kind[i] for i in rec.outputs} == {int(k) for k in ValueKind})
    b.claim("outputs_every_node_of_the_last_level", lambda w: set(last) <= set(rec.outputs))


def _draw_full(b, with_pufks, pufks_kind, width_set):
    P, rng, rec = b.P, b.rng, b.rec
    log_n = P.N.bit_length() - 1
    s, t = _sources(b, 6, 3, 4, 2, 2)
    G, S, V = s[GL], s[GG], s[GV]

    # ---- conversions: SampleExtract / KeyswitchL1toL0 heads and the selectors of every origin
    # (cbs_a and cbs_b head the longest path of the circuit, below: the planner cannot move them, and every circuit bootstrap
    # that is ready by their level runs with them)
    se0 = b.op(FheOp.SampleExtract, [G[0]], b.index())
    cbs_a = b.op(FheOp.CircuitBootstrap, [b.op(FheOp.KeyswitchL1toL0, [se0])])
    uni_one = [b.op(TableOp.PBS_UNIVARIATE, [x, G[2]]) for x in s[L0]]       # ONE table, ready at once, uni_one[3] needed at once
    cbs_b = b.op(FheOp.CircuitBootstrap, [b.op(FheOp.KeyswitchL1toL0, [uni_one[3]])])
    ks_out = b.op(FheOp.KeyswitchL1toL0, [s[L1][0]])        # also an output; two users: a bootstrap now, table bootstraps late
    se_out = b.op(FheOp.SampleExtract, [G[1]], b.index())   # also an output
    cbs_c = [b.op(FheOp.CircuitBootstrap, [ks_out]), b.op(FheOp.CircuitBootstrap, [b.op(FheOp.KeyswitchL1toL0, [se_out])])]
    glev_sel = b.op(FheOp.GlevCMux, [S[0], V[0], V[1]])
    sel_ss = b.op(FheOp.SchemeSwitch, [glev_sel])
    b.keep += [ks_out, se_out, glev_sel, sel_ss, cbs_a]
    b.claim("sample_extract_is_also_an_output", lambda v: se_out in rec.outputs and v.users[se_out])
    b.claim("keyswitch_is_also_an_output", lambda v: ks_out in rec.outputs and v.users[ks_out])
    selectors = S + [t[GG, 0], t[GG, 1], cbs_a, cbs_b, sel_ss] + cbs_c

    # ---- blind rotation: accumulators of level 0, so every chain starts on level 1
    stride = min(2, log_n - 3)                             # 3 bits + stride within log2 N at N = 16
    x_chain = b.rotation(G[2], [S[0], t[GG, 1]])
    y_chain = b.rotation(G[3], [S[0], t[GG, 1]])
    w_chain = b.rotation(G[4], [S[1], t[GG, 0]])
    one_bit = b.rotation(G[5], [t[GG, 1]], stride)
    three = b.rotation(G[2], [cbs_a, sel_ss, S[1]], stride)
    four = b.rotation(G[3], [S[0], cbs_b, t[GG, 0], sel_ss])
    mid_user = b.op(FheOp.Not, [three[1]])
    b.keep += [x_chain[-1], y_chain[-1], w_chain[-1], one_bit[-1], three[-1], four[-1], mid_user]
    for chain in (one_bit, x_chain, three, four):
        b.claim(f"rotation_bits_{len(chain)}", lambda v, chain=chain: all(rec.inputs[m][1] == m - 1 for m in chain[1:]))
    b.claim("rotation_log_stride_0", lambda v: rec.param[four[0]] == 1)
    b.claim("rotation_log_stride_larger", lambda v: stride > 0)
    b.claim("rotation_chains_share_selectors", lambda v: all(v.one_group([x_chain[i], y_chain[i]]) for i in range(2)))
    b.claim("rotation_chains_distinct_selectors", lambda v: all(v.one_group([x_chain[i], w_chain[i]]) for i in range(2)))
    b.claim("rotation_two_rotations_on_one_level", lambda v: v.level[one_bit[0]] == v.level[x_chain[0]] and rec.param[one_bit[0]] != rec.param[x_chain[0]])
    origin = {"input": -1, "trivial": -2, "circuit_bootstrap": int(FheOp.CircuitBootstrap), "scheme_switch_of_glev_cmux": int(FheOp.SchemeSwitch)}
    for name, op in origin.items():
        b.claim(f"rotation_selector_{name}", lambda v, op=op: any(rec.op[rec.inputs[m][0]] == op for m in three + four))
    b.claim("rotation_middle_step_used_elsewhere", lambda v: rec.op[three[1]] == NODE_ROT_CMUX and len(v.users[three[1]]) >= 2)

    # ---- unpack and pack
    w_a, w_b = 2, 3
    n_a, n_b = b.op(FheOp.Not, [G[0]]), b.op(FheOp.Not, [G[1]])          # two rows of one group: consecutive sources
    un_c = [b.unpack(n_a, w_a), b.unpack(n_b, w_a)]
    un_other = b.unpack(n_a, w_b)
    un_s = [b.unpack(G[4], w_a), b.unpack(G[1], w_a)]                      # inputs in descending order: scattered sources
    pack_1 = b.pack([G[5]])
    pack_2 = [b.pack([G[0], n_a]), b.pack([n_b, n_b])]
    pack_9 = b.pack([G[2], n_a] + b.pick(GL, 7 + int(rng.integers(0, 4))))
    un_p = b.unpack(pack_2[0], w_a)
    b.keep += [pack_1, pack_9, pack_2[1]] + un_c[1] + un_other + un_s[0] + un_p
    b.claim("unpack_two_calls_consecutive_sources", lambda v: v.whole_group(un_c[0] + un_c[1]) and v.rows([n_a, n_b]))
    b.claim("unpack_two_calls_scattered_sources", lambda v: v.whole_group(un_s[0] + un_s[1]))
    b.claim("unpack_two_widths_on_one_level", lambda v: v.level[un_other[0]] == v.level[un_c[0][0]])
    b.claim("unpack_source_is_a_pack", lambda v: rec.op[rec.inputs[un_p[0]][0]] == NODE_PACK)
    b.claim("pack_operands_from_two_levels", lambda v: v.level[G[0]] != v.level[n_a])
    b.claim("pack_operand_repeated", lambda v: len(set(rec.inputs[pack_2[1]])) == 1)
    b.claim("pack_two_of_one_width_on_one_level", lambda v: v.one_group(pack_2))
    b.claim("pack_width_1", lambda v: len(rec.inputs[pack_1]) == 1)
    b.claim("pack_width_2", lambda v: len(rec.inputs[pack_2[0]]) == 2)
    b.claim("pack_width_above_8", lambda v: len(rec.inputs[pack_9]) > 8)

    # ---- the CMUX family: a base on one level, then levels of the drawn widths, each reading the level before it
    base = [b.op(FheOp.Not, [b.op(FheOp.MulXN, [b.op(FheOp.GlweAdd, [G[i], G[i + 1]])], int(rng.integers(0, 2 * P.N)))]) for i in (0, 2)]
    base += [b.op(FheOp.GlweAdd, [x_chain[-1], n_a]), b.op(FheOp.MulXN, [w_chain[-1]], int(rng.integers(0, 2 * P.N)))]
    assert {b.lvl[i] for i in base} == {3} and all(b.lvl[q] <= 3 for q in selectors)
    # a circuit bootstrap that is ready after cbs_a's level and first needed in the last level
    cbs_early = b.op(FheOp.CircuitBootstrap, [b.op(FheOp.KeyswitchL1toL0, [b.op(FheOp.SampleExtract, [y_chain[-1]], b.index())])])
    widths = list(width_set) + [2, 3, 1][len(width_set) - 2:]
    prev, glev_prev, levels = base, V[0], []
    for depth, width in enumerate(widths):
        last_level = depth == len(widths) - 1
        older = b.older(GL, b.lvl[prev[0]])
        # the longest path runs through the first node of every level; at its head both early circuit bootstraps
        sel = cbs_a if depth == 0 else b.pick(GG, among=selectors)
        trio = [b.op(FheOp.CMux, [sel, prev[0], prev[1]]), b.op(FheOp.GlevCMux, [sel, glev_prev, t[GV, depth % 2]]),
                b.op(FheOp.MultiplyGgswGlwe, [sel, prev[0]])]
        if depth == 0:
            b.claim("cmux_glev_cmux_and_multiply_share_a_selector_on_one_level", lambda v, trio=trio: len({v.level[i] for i in trio}) == 1)
        glev_prev = trio[1]
        new = [trio[0]]
        if depth == 0:
            new.append(b.op(FheOp.CMux, [cbs_b, prev[1], G[5]]))
        if last_level:                                      # the two late selectors select something
            new += [b.op(FheOp.CMux, [q, b.pick(GL, among=prev), b.pick(GL, among=older)]) for q in (cbs_early, cbs_late)]
        while len(new) < width:
            new.append(b.op(FheOp.CMux, [b.pick(GG, among=selectors), b.pick(GL, among=prev), b.pick(GL, among=older)]))
        others = [b.op(FheOp.Not, [b.pick(GL, among=prev)])]
        if depth in (0, 2):
            others += [b.op(FheOp.GlweAdd, [b.pick(GL, among=prev), b.pick(GL, among=older)]),
                       b.op(FheOp.MulXN, [b.pick(GL, among=prev)], int(rng.integers(0, 2 * P.N)))]
        levels.append(new)
        b.claim(f"cmux_width_{len(new)}", lambda v, new=new: v.whole_group(new))
        if depth == 0:      # conversions in the middle of the graph: ready late, used next to the early one in the last level
            se_mid = b.op(FheOp.SampleExtract, [new[-1]], b.index())   # two users, which the planner pulls to different levels
            cbs_late = b.op(FheOp.CircuitBootstrap, [b.op(FheOp.KeyswitchL1toL0, [se_mid])])
            uni_lwe_late = b.op(FheOp.KeyswitchL1toL0, [se_mid])
        prev = new + [trio[2]] + others
    b.keep += [glev_prev]
    b.claim("slack_circuit_bootstrap_early_next_to_late", lambda v: v.moved_next_to_late(cbs_early, cbs_late))

    # ---- table bootstraps.  tables: inputs, and values computed in the last level (later than every LWE operand)
    deep = levels[-1]
    t_late = [b.op(FheOp.MulXN, [deep[0]], int(rng.integers(1, 2 * P.N))), deep[-1]]    # a MulXN and a CMux result
    uni_late = b.op(TableOp.PBS_UNIVARIATE, [uni_lwe_late, G[2]])    # ready in the middle, not needed: run with the last ones
    ks_rows = [b.op(FheOp.KeyswitchL1toL0, [u]) for u in uni_one[:3]]                   # one keyswitch group: consecutive rows
    p_mid = int(rng.integers(1, 63))
    biv_c = [b.op(TableOp.PBS_BIVARIATE, [ks_rows[i], ks_rows[i + 1], G[3]], p_mid) for i in (0, 1)]
    biv_s = [b.op(TableOp.PBS_BIVARIATE, [ks_rows[i], x, G[2]], 0) for i, x in ((0, s[L0][3]), (1, t[L0, 1]))]
    biv_same = [b.op(TableOp.PBS_BIVARIATE, [x, x, t_late[0]], 63) for x in (ks_out, s[L0][0])]
    uni_each = [b.op(TableOp.PBS_UNIVARIATE, [x, tab]) for x, tab in zip((s[L0][1], t[L0, 0], ks_out), (t_late[0], t_late[1], t_late[0]))]
    b.keep += uni_one + [uni_late] + ks_rows + biv_c + biv_s + biv_same + uni_each
    b.claim("pbs_group_one_table", lambda v: v.whole_group(uni_one))
    b.claim("pbs_group_tables_out_of_order", lambda v: v.one_group(uni_each) and rec.inputs[uni_each[0]][1] > rec.inputs[uni_each[1]][1])
    b.claim("pbs_table_computed_later_than_its_lwes", lambda v: all(v.level[rec.inputs[u][1]] > v.level[rec.inputs[u][0]] for u in uni_each)
            and rec.op[t_late[0]] == int(FheOp.MulXN) and rec.op[t_late[1]] == int(FheOp.CMux))
    b.claim("pbs_univariate_and_bivariate_on_one_level", lambda v: v.level[uni_each[0]] == v.level[biv_same[0]])
    b.claim("bivariate_both_inputs_consecutive", lambda v: v.whole_group(biv_c) and v.rows(ks_rows))
    b.claim("bivariate_one_input_scattered", lambda v: v.whole_group(biv_s) and v.rows(ks_rows[:2]) and not v.one_group([s[L0][3], t[L0, 1]]))
    b.claim("bivariate_same_node_twice", lambda v: v.whole_group(biv_same))
    b.claim("bivariate_plaintext_bits_0", lambda v: rec.param[biv_s[0]] == 0)
    b.claim("bivariate_plaintext_bits_middle", lambda v: 0 < p_mid < 63)
    b.claim("bivariate_plaintext_bits_63", lambda v: rec.param[biv_same[0]] == 63)
    b.claim("slack_univariate_early_next_to_late", lambda v: v.moved_next_to_late(uni_late, uni_each[0]))
    b.claim("slack_bivariate_early_next_to_late", lambda v: v.moved_next_to_late(biv_c[0], biv_same[0]))
    b.claim("sample_extract_users_on_two_levels", lambda v: len(v.user_levels(se_mid)) > 1)
    b.claim("keyswitch_users_on_two_levels", lambda v: len(v.user_levels(ks_out)) > 1)

    # ---- public functional keyswitch: ONE operand kind in a circuit (a context holds one such key)
    if with_pufks:
        kind = ValueKind(pufks_kind)
        if kind == L0:
            pair = [b.op(FheOp.KeyswitchL1toL0, [s[L1][i]]) for i in (1, 2)]            # one keyswitch group's outputs
            rows = s[L0] + [t[L0, 0], t[L0, 1], ks_out] + pair       # (not ks_rows: a user down here would hold one of them back)
        else:
            pair = b.unpack(G[3], w_b)[:2]                           # the first bits of one unpack call
            rows = s[L1] + [t[L1, 0], t[L1, 1], se0, se_out] + un_s[1] + uni_one + pair   # (level 1 at most: the CMux below
            #                                                                               stays under the levels above)
        large = min(P.N, 33 + int(rng.integers(0, 8)))
        k_pair = b.pufks(pair)
        k_one = b.pufks([b.pick(kind, among=rows)])
        drawn = b.pick(kind, large - 1, among=rows)
        drawn.insert(int(rng.integers(1, large)), drawn[0])
        k_large = [b.pufks(drawn), b.pufks([drawn[int(i)] for i in rng.permutation(large)])]
        as_table = b.op(TableOp.PBS_UNIVARIATE, [s[L0][2], k_pair])
        as_operand = b.op(FheOp.CMux, [S[1], k_one, k_large[0]])
        as_source = b.unpack(k_large[1], w_b)
        b.keep += [k_pair, k_one, as_table, as_operand] + k_large + as_source
        b.claim("pufks_rows_consecutive", lambda v: v.whole_group([k_pair]) and v.rows(pair))
        b.claim("pufks_rows_scattered_with_repeats", lambda v: len(set(drawn)) < len(drawn) and len({v.level[i] for i in drawn}) > 1)
        b.claim("pufks_count_1", lambda v: len(rec.inputs[k_one]) == 1)
        b.claim("pufks_count_2", lambda v: len(rec.inputs[k_pair]) == 2)
        b.claim("pufks_count_large", lambda v: len(rec.inputs[k_large[0]]) >= min(P.N, 33))
        b.claim("pufks_two_of_one_count_on_one_level", lambda v: v.whole_group(k_large))
        b.claim("pufks_result_as_table", lambda v: rec.op[rec.inputs[as_table][1]] == NODE_PUFKS)
        b.claim("pufks_result_as_cmux_operand", lambda v: all(rec.op[j] == NODE_PUFKS for j in rec.inputs[as_operand][1:]))
        b.claim("pufks_result_as_unpack_source", lambda v: rec.op[rec.inputs[as_source[0]][0]] == NODE_PUFKS)
        b.claim("unpack_source_is_a_keyswitch_node", lambda v: rec.op[rec.inputs[as_source[0]][0]] == NODE_PUFKS)
        # ---- plaintext linear maps: like the keyswitch above they have no submit by handle, so `pushable` draws none
        _draw_linear(b, s, t, G, uni_one, base, levels, p_mid, ValueKind(pufks_kind))
    # ---- polynomial linear maps and the GLWE keyswitch family, from a generator of their own: `pushable` draws the three modes
    # (submits by handle since the pool learned them) and no polynomial layer (there is no submit by handle for one)
    if b.glwe:
        _draw_glwe(b, s, t, levels[0], base, (x_chain, y_chain), cbs_early, p_mid, with_poly=with_pufks)


def _draw_glwe(b, s, t, cmux0, base, chains, cbs_early, p_mid, with_poly):
    """every name of GLWE_PATTERNS (`with_poly`: else GLWE_PUSHABLE_PATTERNS), drawn last.  Nothing here lengthens the graph, no
    bootstrap with a user is added, and the two table bootstraps it adds are ready late and have no users (the slack pass takes
    its leads by latest level, so they lead nobody).  Every layout of a mode stands on a level of its own — (level, operation,
    parameter) is the group key, and a trace has no parameter — so that each claim is about ONE whole group:
      1 over inputs, one of them twice       2 over a pack group (5), other slots / rounds over four of those rows
      3 over the last steps of two rotation chains      4 over two rows of one group in descending order
      5 over four rows of the widest CMUX level         6 over the level-5 group of the same mode
      7 one node of each mode over ONE node             9 over two rows of a 9-row polynomial layer (level 8)
      top: one scattered keyswitch group, and one polynomial layer in place (the last polynomial group in key order: its slot is
      the last id), over four XORs made for them"""
    P, rec, rng = b.P, b.rec, b.grng
    G, S = s[GL], s[GG]
    log_n = P.N.bit_length() - 1
    top = max(b.lvl)
    assert top >= 10 and len(cmux0) >= 16 and all(b.lvl[i] == 3 for i in base[:2]), (top, len(cmux0))
    KSW, AUT, TRC = GLWE_KS_KINDS
    x_chain, y_chain = chains
    only = b.ginp(GL)                                       # an input that reaches the outputs through the new kinds only
    packs = [b.pack([G[(i + j) % 6] for j in range(3)]) for i in range(5)]      # level 1: one group of five
    at = 2 + int(rng.integers(0, len(cmux0) - 14))          # twelve successive rows of the widest CMUX level

    def par(kind):
        """a drawn parameter: one of the two trace-radix slots, any round, nothing"""
        return (K_A, K_B)[int(rng.integers(0, 2))] if kind == KSW else int(rng.integers(1, log_n + 1)) if kind == AUT else 0

    def group(kind, param, operands):
        return [b.glwe_node(kind, param, x) for x in operands]

    def whole_in_place(nodes, op=None):
        return lambda v: v.whole_group(nodes) and v.in_place(nodes[0]) and (op is None or all(rec.op[rec.inputs[n][0]] == op for n in nodes))

    lv = {}                                                 # mode -> {level: its group}
    for mode, kind in GLWE_MODES:
        g = lv[mode] = {}
        g[1] = group(kind, par(kind), [G[0], only, only, G[5]])
        g[2] = group(kind, {KSW: K_A, AUT: 1, TRC: 0}[kind], packs)
        g[3] = group(kind, par(kind), [x_chain[-1], y_chain[-1]])
        g[4] = group(kind, par(kind), [base[1], base[0]])
        g[5] = group(kind, par(kind), cmux0[at:at + 4])
        g[6] = group(kind, par(kind), g[5])
        b.claim(f"glwe_{mode}_scattered_with_a_repeat", lambda v, n=g[1]: v.whole_group(n) and v.scattered(v.linear_operands(n[0]))
                and len(set(v.linear_operands(n[0]))) < len(n))
        b.claim(f"glwe_{mode}_in_place_over_a_pack_group", whole_in_place(g[2], NODE_PACK))
        b.claim(f"glwe_{mode}_group_of_5", lambda v, n=g[2]: v.whole_group(n) and len(n) == 5)
        b.claim(f"glwe_{mode}_in_place_over_rotation_chains", whole_in_place(g[3], NODE_ROT_CMUX))
        b.claim(f"glwe_{mode}_scattered_descending", lambda v, n=g[4]: v.whole_group(n) and len(set(v.linear_operands(n[0]))) == len(n)
                and v.position(rec.inputs[n[1]][0]) < v.position(rec.inputs[n[0]][0]))
        b.claim(f"glwe_{mode}_in_place_over_a_cmux_group", whole_in_place(g[5], int(FheOp.CMux)))
        b.claim(f"glwe_{mode}_group_of_4", lambda v, n=g[5]: v.whole_group(n) and len(n) == 4)
        b.claim(f"glwe_{mode}_in_place_over_its_own_mode", whole_in_place(g[6], kind))
    # further slots and rounds on level 2, over four of the five pack rows; the other-radix slot scattered on level 1 as well
    ks_b, ks_other, au_last = group(KSW, K_B, packs[1:]), group(KSW, K_OTHER, packs[:4]), group(AUT, log_n, packs[1:])
    other_scattered = group(KSW, K_OTHER, [G[3], G[1], G[3]])
    b.claim("glwe_two_keyswitch_slots_on_one_level", lambda v: v.level[ks_b[0]] == v.level[lv["keyswitch"][2][0]] and whole_in_place(ks_b)(v)
            and whole_in_place(lv["keyswitch"][2])(v))
    b.claim("glwe_other_radix_slot_and_trace_radix_slot_on_one_level", lambda v: v.level[ks_other[0]] == v.level[ks_b[0]] and whole_in_place(ks_other)(v)
            and v.whole_group(other_scattered) and v.scattered(v.linear_operands(other_scattered[0])))
    b.claim("glwe_two_automorphism_rounds_on_one_level", lambda v: v.level[au_last[0]] == v.level[lv["automorphism"][2][0]] and whole_in_place(au_last)(v)
            and (log_n == 1 or rec.param[au_last[0]] != rec.param[lv["automorphism"][2][0]]))
    b.claim("glwe_automorphism_round_1", lambda v: rec.param[lv["automorphism"][2][0]] == 1)
    b.claim("glwe_automorphism_round_log2_n", lambda v: rec.param[au_last[0]] == log_n)
    # one node of each mode over ONE node, the first row of the trace of traces
    x_one = lv["trace"][6][0]
    one = {mode: group(kind, par(kind), [x_one]) for mode, kind in GLWE_MODES}
    for mode, _ in GLWE_MODES:
        b.claim(f"glwe_{mode}_group_of_1", lambda v, n=one[mode]: v.whole_group(n))
    b.claim("glwe_all_three_modes_over_one_operand_on_one_level", lambda v: len({v.level[n[0]] for n in one.values()}) == 1
            and {rec.inputs[n[0]] for n in one.values()} == {(x_one,)})
    b.claim("glwe_input_reaches_the_outputs_through_the_new_kinds_only", lambda v: v.users[only] and all(rec.op[u] in GLWE_KS_KINDS + (NODE_GLWE_POLY_LINEAR,) for u in v.users[only]))

    # ---- the last launches: four XORs on the level below the top, made last of their group, so successive rows
    x = one["automorphism"][0]
    while b.lvl[x] < top - 2:
        x = b.op(FheOp.Not, [x])
    raised = [b.op(FheOp.GlweAdd, [x, G[i]]) for i in range(4)]
    last_ks = group(KSW, K_A, [raised[2], raised[0], raised[2]])
    b.claim("glwe_last_keyswitch_group_scattered", lambda v: v.whole_group(last_ks) and v.scattered(v.linear_operands(last_ks[0]))
            and v.level[last_ks[0]] > max(v.level[i] for i, op in enumerate(rec.op) if op in GLWE_KS_KINDS and i not in last_ks))

    # ---- consumers of the new rows
    tr1, tr2, ks1, au1 = lv["trace"][1], lv["trace"][2], lv["keyswitch"][1], lv["automorphism"][1]
    bits = b.unpack(tr2[0], 2)
    se_two = b.op(FheOp.SampleExtract, [tr2[1]], int(rng.integers(0, P.N)))
    ks_of_se = b.op(FheOp.KeyswitchL1toL0, [se_two])
    packed = b.pack([tr1[0], ks1[0], au1[1]])
    cm = b.op(FheOp.CMux, [S[0], ks1[1], au1[2]])
    rot = b.rotation(tr1[3], [S[1]])
    p_free = 40 if p_mid != 40 else 41          # plaintext bits of a bivariate group of its own (0, 63, p_mid and 1 .. 3 are taken)
    uni = b.op(TableOp.PBS_UNIVARIATE, [s[L0][0], tr2[2]])
    biv = b.op(TableOp.PBS_BIVARIATE, [s[L0][1], s[L0][0], lv["automorphism"][2][0]], p_free)
    b.keep += [ks_of_se, packed, cm, rot[-1], uni, biv] + bits
    is_new = lambda n: rec.op[n] in GLWE_KS_KINDS
    b.claim("glwe_result_as_unpack_source", lambda v: is_new(rec.inputs[bits[0]][0]))
    b.claim("glwe_result_into_a_sample_extract_and_a_keyswitch", lambda v: is_new(rec.inputs[se_two][0]) and rec.inputs[ks_of_se] == (se_two,))
    b.claim("glwe_result_as_pack_operand", lambda v: all(is_new(n) for n in rec.inputs[packed]) and len({rec.op[n] for n in rec.inputs[packed]}) == 3)
    b.claim("glwe_results_as_cmux_low_and_high", lambda v: all(is_new(n) for n in rec.inputs[cm][1:]))
    b.claim("glwe_result_as_rotation_accumulator", lambda v: rec.op[rot[0]] == NODE_ROT_CMUX and is_new(rec.inputs[rot[0]][1]))
    b.claim("glwe_result_as_univariate_table", lambda v: is_new(rec.inputs[uni][1]))
    b.claim("glwe_result_as_bivariate_table", lambda v: is_new(rec.inputs[biv][2]) and v.whole_group([biv]))
    if not with_poly:
        return

    # ---- polynomial layers
    layer = b.poly_linear
    slot_of = lambda nodes: rec.linear_of(nodes[0])[0]
    cls_of = lambda nodes: GLWE_POLY_CLASS[slot_of(nodes)]
    q_pack = layer(P_B, packs[:4])                                              # level 2
    q_rows = [layer(P_ROW, packs), layer(P_ROW, [packs[4], packs[1], packs[0], packs[2], packs[2]])]
    q_prev, q_ks = layer(P_A, q_pack), layer(P_B, au_last)                      # level 3
    q_empty = layer(P_EMPTY, [q_pack[3], q_pack[0], tr2[1], G[1], q_pack[0]])
    perm = [q_prev[int(i)] for i in rng.permutation(4)]
    if perm == q_prev:
        perm = perm[::-1]
    q_perm, q_twice = layer(P_A, perm), layer(P_B, [q_prev[0], q_prev[1], q_prev[1], q_prev[3]])      # level 4
    q_two = [layer(P_A, cmux0[at:at + 4]), layer(P_A, cmux0[at + 4:at + 8])]  # level 5
    q_cmux = layer(P_B, cmux0[at + 8:at + 12])
    q_mixed = layer(P_WIDE, [cmux0[at], q_pack[2], G[4], t[GL, 1], t[GL, 0], packs[3], only])
    q_one = layer(P_ONE, [x_one])                                               # level 7
    mul = b.op(FheOp.MultiplyGgswGlwe, [cbs_early, G[0]])   # ready early; runs behind the moved circuit bootstrap
    q_moved = layer(P_UNIT, [mul])
    q_tall = layer(P_TALL, [one["keyswitch"][0], one["trace"][0]])              # level 8: rows 0 and 1 are read, the rest is dead
    over_tall = {mode: group(kind, par(kind), q_tall[:2]) for mode, kind in GLWE_MODES}  # level 9
    q_last = layer(P_A, raised)                                                 # the top
    b.dead |= set(q_tall[2:])
    b.keep += q_pack
    for mode, _ in GLWE_MODES:
        b.claim(f"glwe_{mode}_in_place_over_a_polynomial_layer", whole_in_place(over_tall[mode], NODE_GLWE_POLY_LINEAR))
    b.claim("poly_in_place_over_a_pack_group", lambda v: whole_in_place(q_pack, NODE_PACK)(v))
    b.claim("poly_in_place_over_a_previous_layer", lambda v: v.whole_group(q_prev) and v.in_place(q_prev[0]) and rec.inputs[q_prev[0]] == tuple(q_pack))
    b.claim("poly_in_place_over_a_keyswitch_group", lambda v: v.whole_group(q_ks) and v.in_place(q_ks[0]) and all(is_new(n) for n in rec.inputs[q_ks[0]]))
    b.claim("poly_in_place_over_a_cmux_group", lambda v: v.whole_group(q_cmux) and v.in_place(q_cmux[0]) and all(rec.op[n] == int(FheOp.CMux) for n in rec.inputs[q_cmux[0]]))
    b.claim("poly_two_layers_in_place", lambda v: v.whole_group(q_two[0] + q_two[1]) and v.in_place(q_two[0][0]) and v.rows(cmux0[at:at + 8]))
    b.claim("poly_scattered_previous_layer_permuted", lambda v: v.whole_group(q_perm) and v.scattered(rec.inputs[q_perm[0]])
            and sorted(rec.inputs[q_perm[0]]) == q_prev)
    b.claim("poly_scattered_operand_repeated", lambda v: v.whole_group(q_twice) and v.scattered(rec.inputs[q_twice[0]])
            and len(set(rec.inputs[q_twice[0]])) == 3)
    b.claim("poly_scattered_three_levels_inputs_and_constants", lambda v: v.whole_group(q_mixed) and v.scattered(rec.inputs[q_mixed[0]])
            and len({v.level[j] for j in rec.inputs[q_mixed[0]]}) >= 4 and {rec.op[j] for j in rec.inputs[q_mixed[0]]} >= {-1, -2}
            and {(rec.kind[j], rec.param[j]) for j in rec.inputs[q_mixed[0]] if rec.op[j] == -2} == {(int(GL), 0), (int(GL), 1)})
    b.claim("poly_two_layers_one_consecutive_one_scattered", lambda v: v.whole_group(q_rows[0] + q_rows[1]) and v.rows(list(rec.inputs[q_rows[0][0]]))
            and v.scattered(rec.inputs[q_rows[1][0]]) and not v.in_place(q_rows[0][0]))
    b.claim("poly_two_slots_of_one_shape_on_one_level", lambda v: v.level[q_prev[0]] == v.level[q_ks[0]] and slot_of(q_prev) != slot_of(q_ks)
            and GLWE_POLY_SHAPE[slot_of(q_prev)] == GLWE_POLY_SHAPE[slot_of(q_ks)] and v.whole_group(q_prev) and v.whole_group(q_ks))
    b.claim("poly_constants_only_in_place", lambda v: cls_of(q_pack) == "constants" and v.in_place(q_pack[0]))
    b.claim("poly_general_in_place", lambda v: cls_of(q_prev) == "general" and v.in_place(q_prev[0]))
    b.claim("poly_constants_only_scattered", lambda v: cls_of(q_twice) == "constants" and v.scattered(v.linear_operands(q_twice[0])))
    b.claim("poly_general_scattered", lambda v: cls_of(q_perm) == "general" and v.scattered(v.linear_operands(q_perm[0])))
    b.claim("poly_empty_matrix_with_a_bias", lambda v: cls_of(q_empty) == "empty" and v.whole_group(q_empty) and v.scattered(rec.inputs[q_empty[0]]))
    b.claim("poly_shape_1_1", lambda v: GLWE_POLY_SHAPE[slot_of(q_one)] == (1, 1) and v.whole_group(q_one) and v.in_place(q_one[0]))
    b.claim("poly_follows_a_cmux_on_a_moved_circuit_bootstrap", lambda v: v.asap[cbs_early] + 2 <= v.level[cbs_early] == v.level[mul] - 1
            and v.level[q_moved[0]] == v.level[mul] + 1 > v.asap[q_moved[0]] and v.whole_group(q_moved))
    b.claim("poly_layer_partly_used", lambda v: len(q_tall) == 9 and all(v.users[n] for n in q_tall[:2])
            and not any(v.users[n] or n in rec.outputs for n in q_tall[2:]))
    b.claim("poly_row_is_an_output_and_has_users", lambda v: all(n in rec.outputs and v.users[n] for n in q_pack))
    b.claim("poly_over_results_of_the_keyswitch_family", lambda v: {rec.op[n] for n in rec.inputs[q_tall[0]]} == {KSW, TRC})
    b.claim("poly_last_group_in_place_general", lambda v: cls_of(q_last) == "general" and v.whole_group(q_last) and v.in_place(q_last[0])
            and v.key(q_last[0]) == max(v.key(i) for i, op in enumerate(rec.op) if op == NODE_GLWE_POLY_LINEAR))

    # ---- sample extracts of trace results next to the LWE linear layers (profile `full` has their weight slots): one with users
    # on two levels, and one that is ready on level 2 and first used by a layer above level 7, created right after a late head of
    # its own group — the layer's two rows are consecutive only because the head was pulled up
    index = int(rng.integers(0, P.N))
    deep, early = b.op(FheOp.SampleExtract, [lv["trace"][6][1]], index), b.op(FheOp.SampleExtract, [tr1[1]], index)
    pulled = b.linear(S_PAIR, [deep, early])
    both = b.linear(S_TWICE, [se_two, deep])
    b.claim("glwe_sample_extract_users_on_two_levels", lambda v: len(v.user_levels(se_two)) > 1 and is_new(rec.inputs[se_two][0]))
    b.claim("glwe_pulls_a_sample_extract_up", lambda v: v.asap[early] + 2 <= v.level[pulled[0]] and v.level[early] == v.level[pulled[0]] - 1
            and v.level[pulled[0]] == min(v.user_levels(early)) and v.whole_group(pulled) and v.in_place(pulled[0]) and is_new(rec.inputs[early][0]))


def _draw_linear(b, s, t, G, uni_one, base, cmux_levels, p_mid, pufks_kind):
    """every name of LINEAR_PATTERNS, drawn last: nothing here lengthens the graph (the deepest node stands on its last level)
    and nothing takes slack from a bootstrap above (the deep sources are nodes of the longest path, which have none)"""
    rec, rng = b.rec, b.rng
    KS, SE, UNI, BIV = FheOp.KeyswitchL1toL0, FheOp.SampleExtract, TableOp.PBS_UNIVARIATE, TableOp.PBS_BIVARIATE
    top = max(b.lvl)
    slot_of = lambda layer: rec.linear_of(layer[0])[0]

    # ---- level 2: layers over ONE keyswitch group (level 0 rows) and over the one-table bootstrap group (level 1 rows)
    ks = [b.op(KS, [b.inp(L1)]) for _ in range(10)]           # users: layers of level 2 first, so the rows stay on level 1
    a_ks, b_ks, a_pbs = b.linear(S_A, ks[:4]), b.linear(S_B, ks[:4]), b.linear(S_A, uni_one)
    wide = [b.linear(S_WIDE, ks[4:7]), b.linear(S_WIDE, ks[7:10])]
    mixed = [b.linear(S_BITS, uni_one[:3]), b.linear(S_BITS, [uni_one[3], uni_one[1], uni_one[0]])]
    twice = [b.linear(S_TWICE, ks[8:10]) for _ in range(2)]
    b.claim("linear_in_place_over_a_keyswitch_group", lambda v: v.whole_group(a_ks) and v.in_place(a_ks[0]) and rec.inputs[a_ks[0]] == tuple(ks[:4]))
    b.claim("linear_in_place_over_a_univariate_group", lambda v: v.whole_group(a_pbs) and v.in_place(a_pbs[0]) and v.whole_group(uni_one))
    b.claim("linear_two_layers_in_place", lambda v: v.whole_group(wide[0] + wide[1]) and v.in_place(wide[0][0]) and v.rows(ks[4:10]))
    b.claim("linear_two_layers_one_consecutive_one_scattered", lambda v: v.whole_group(mixed[0] + mixed[1]) and v.rows(list(rec.inputs[mixed[0][0]]))
            and v.scattered(rec.inputs[mixed[1][0]]) and not v.in_place(mixed[0][0]))
    b.claim("linear_two_layers_over_one_operand_list", lambda v: v.whole_group(twice[0] + twice[1]) and rec.inputs[twice[0][0]] == rec.inputs[twice[1][0]]
            and v.scattered(v.linear_operands(twice[0][0])))
    b.claim("linear_two_slots_of_one_shape_on_one_level", lambda v: v.level[a_ks[0]] == v.level[b_ks[0]] and v.whole_group(a_ks) and v.whole_group(b_ks)
            and LINEAR_SHAPE[S_A] == LINEAR_SHAPE[S_B] and rec.kind[a_ks[0]] == rec.kind[b_ks[0]] and v.in_place(b_ks[0]))
    b.claim("linear_both_operand_kinds_on_one_level_with_one_slot", lambda v: v.level[a_ks[0]] == v.level[a_pbs[0]] and slot_of(a_ks) == slot_of(a_pbs)
            and {rec.kind[a_ks[0]], rec.kind[a_pbs[0]]} == {int(L0), int(L1)})

    # ---- the planner: conversion heads that are ready early and first used by a layer far above, next to a late one of their
    # own group and created right after it: the layer's two rows are consecutive only because the head was pulled up
    index = b.index()
    deep_l0, ks_early = b.op(KS, [b.op(SE, [base[1]], b.index())]), b.op(KS, [b.inp(L1)])
    pl_ks = b.linear(S_PAIR, [deep_l0, ks_early])
    deep_l1, se_early = b.op(SE, [cmux_levels[0][0]], index), b.op(SE, [G[3]], index)
    pl_se = b.linear(S_PAIR, [deep_l1, se_early])
    for name, head, layer in (("keyswitch", ks_early, pl_ks), ("sample_extract", se_early, pl_se)):
        b.claim(f"linear_pulls_a_{name}_up", lambda v, head=head, layer=layer: v.asap[head] + 2 <= v.level[layer[0]] and v.level[head] == v.level[layer[0]] - 1
                and v.level[layer[0]] == min(v.user_levels(head)) and v.whole_group(layer) and v.in_place(layer[0]))
    # a table bootstrap that is ready on level 2 and has slack, next to one that is ready on level 4 and has none (a public
    # functional keyswitch and a chain of Not up to the last level hang on it): the slack pass runs both on level 4, and a layer
    # whose other operand is an input follows the early one
    ks_lin = [b.op(KS, [x]) for x in a_pbs[:2]]
    uni_e, uni_l = b.op(UNI, [ks[6], G[2]]), b.op(UNI, [ks_lin[0], G[2]])
    x = b.pufks([uni_l] if pufks_kind == L1 else [b.op(KS, [uni_l])])
    while b.lvl[x] < top:
        x = b.op(FheOp.Not, [x])
    pl_uni = b.linear(S_PAIR, [uni_e, s[L1][0]])
    b.keep += [x]
    b.claim("linear_follows_a_moved_table_bootstrap", lambda v: v.moved_next_to_late(uni_e, uni_l) and v.level[pl_uni[0]] == v.level[uni_e] + 1 > v.asap[pl_uni[0]])
    b.claim("linear_rows_into_a_keyswitch", lambda v: all(rec.op[rec.inputs[k][0]] == NODE_LWE_LINEAR and rec.kind[rec.inputs[k][0]] == int(L1) for k in ks_lin))

    # ---- scattered
    perm = [a_ks[int(i)] for i in rng.permutation(len(a_ks))]
    if perm == a_ks:
        perm = perm[::-1]
    only_linear = b.inp(L0)                                   # an input that reaches the outputs through a linear layer only
    lists = {"previous_layer_permuted": (S_PERM, perm),
             "operand_repeated": (S_REPEAT, [ks[1], ks[3], ks[1], wide[1][2], b_ks[7]]),
             "three_levels_inputs_and_constants": (S_MIXED, [deep_l0, a_ks[2], ks[5], only_linear, t[L0, 1], t[L0, 0], s[L0][2]])}
    sc = {name: b.linear(slot, ops) for name, (slot, ops) in lists.items()}
    also = {"previous_layer_permuted": lambda v, ops: sorted(ops) == a_ks and ops != a_ks,
            "operand_repeated": lambda v, ops: len(set(ops)) == len(ops) - 1,
            "three_levels_inputs_and_constants": lambda v, ops: len({v.level[j] for j in ops}) >= 4 and {-1, -2} <= {rec.op[j] for j in ops}}
    for name, layer in sc.items():
        b.claim(f"linear_scattered_{name}", lambda v, name=name, layer=layer: v.whole_group(layer) and v.scattered(rec.inputs[layer[0]])
                and also[name](v, list(rec.inputs[layer[0]])))

    # ---- consumers of linear rows
    one = b.linear(S_ONE, [deep_l0])
    cbs = b.op(FheOp.CircuitBootstrap, [one[0]])
    uni_lin = b.op(UNI, [b_ks[0], G[2]])
    # plaintext bits no other bivariate group has, so that each pair is a group of its own: _draw_full's bivariates take 0, 63 and
    # p_mid and nothing else, and a bivariate node is drawn nowhere else (both whole_group claims below would refuse a collision)
    p_c, p_s = [p for p in (1, 2, 3) if p != p_mid][:2]
    biv_c = [b.op(BIV, [a_ks[i], a_ks[i + 1], G[3]], p_c) for i in (0, 1)]
    biv_s = [b.op(BIV, [a_ks[4 + i], x, G[2]], p_s) for i, x in enumerate((t[L0, 1], s[L0][3]))]
    rows = pl_ks if pufks_kind == L0 else pl_se
    k_rows, k_repeat = b.pufks(rows), b.pufks([rows[0], rows[1], rows[1], rows[2]])
    b.dead |= set(wide[1]) - {wide[1][2], wide[1][16]}
    b.keep += a_ks + [wide[1][16], cbs, uni_lin, k_rows, k_repeat] + biv_c + biv_s + sc["three_levels_inputs_and_constants"]
    b.claim("linear_shape_1_1", lambda v: LINEAR_SHAPE[slot_of(one)] == (1, 1) and v.in_place(one[0]))
    b.claim("linear_row_into_a_circuit_bootstrap", lambda v: rec.inputs[cbs] == (one[0],) and rec.kind[one[0]] == int(L0))
    b.claim("linear_row_into_a_univariate_bootstrap", lambda v: rec.inputs[uni_lin][0] == b_ks[0] and rec.kind[b_ks[0]] == int(L0))
    b.claim("linear_rows_into_a_bivariate_consecutive", lambda v: v.whole_group(biv_c) and v.rows(a_ks[:3]))
    b.claim("linear_row_into_a_bivariate_scattered", lambda v: v.whole_group(biv_s) and v.rows(a_ks[4:6]) and v.scattered([rec.inputs[n][1] for n in biv_s]))
    b.claim("linear_rows_into_a_functional_keyswitch_in_order", lambda v: v.whole_group([k_rows]) and v.rows(rows) and rec.inputs[k_rows] == tuple(rows))
    b.claim("linear_rows_into_a_functional_keyswitch_with_a_repeat", lambda v: v.whole_group([k_repeat]) and len(set(rec.inputs[k_repeat])) < len(rec.inputs[k_repeat])
            and all(rec.op[j] == NODE_LWE_LINEAR for j in rec.inputs[k_repeat]))
    b.claim("linear_row_is_an_output_and_has_users", lambda v: all(n in rec.outputs and v.users[n] for n in a_ks[:6]))
    b.claim("linear_layer_partly_used", lambda v: {bool(v.users[n]) or n in rec.outputs for n in wide[1]} == {True, False}
            and v.users[wide[1][2]] and wide[1][16] in rec.outputs)

    # ---- the last linear launch: unpack bits of a deep node, a layer over the first of them, a layer with one-limb weights over
    # all of its rows, alone on the deepest level that has linear nodes (with the matrix cores forced, their kernel is the last)
    bits = b.unpack(cmux_levels[2][0], 5)
    over_bits = b.linear(S_BITS, bits[:3])
    last = b.linear(S_LAST, over_bits)
    b.claim("linear_in_place_over_unpack_bits", lambda v: v.whole_group(over_bits) and v.in_place(over_bits[0]) and rec.param[bits[0]] == 0)
    b.claim("linear_in_place_over_a_previous_layer", lambda v: v.whole_group(last) and v.in_place(last[0]) and rec.inputs[last[0]] == tuple(over_bits))
    b.claim("linear_last_group_in_place_with_one_limb_weights", lambda v: LINEAR_CLASS[slot_of(last)] == 1 and v.whole_group(last) and v.in_place(last[0])
            and v.level[last[0]] > max(v.level[i] for i, op in enumerate(rec.op) if op == NODE_LWE_LINEAR and i not in last))


def _draw_small(b, with_pufks, pufks_kind):
    """every node kind once or twice, nothing wider than 3 but the two linear layers, for random parameter sets"""
    P, rng = b.P, b.rng
    s, t = _sources(b, 3, 1, 2, 1, 1)
    G, S, V = s[GL], s[GG], s[GV]
    se = b.op(FheOp.SampleExtract, [G[0]], b.index())
    l0 = [b.op(FheOp.KeyswitchL1toL0, [se]), b.op(FheOp.KeyswitchL1toL0, [s[L1][0]])]
    cbs = [b.op(FheOp.CircuitBootstrap, [x]) for x in l0]
    glev = b.op(FheOp.GlevCMux, [cbs[0], V[0], t[GV, 1]])
    sel_ss = b.op(FheOp.SchemeSwitch, [glev])
    sels = S + cbs + [sel_ss, t[GG, 0], t[GG, 1]]
    vals = list(G) + [t[GL, 1]]
    for _ in range(2):
        vals += [b.op(FheOp.CMux, [b.pick(GG, among=sels)] + b.pick(GL, 2, among=vals)) for _ in range(int(rng.integers(1, 4)))]
        vals += [b.op(FheOp.Not, [b.pick(GL, among=vals)]), b.op(FheOp.GlweAdd, b.pick(GL, 2, among=vals)),
                 b.op(FheOp.MulXN, [b.pick(GL, among=vals)], int(rng.integers(0, 2 * P.N))),
                 b.op(FheOp.MultiplyGgswGlwe, [b.pick(GG, among=sels), b.pick(GL, among=vals)])]
    n_bits = int(rng.integers(1, 4))
    rot = b.rotation(b.pick(GL, among=vals), b.pick(GG, n_bits, among=sels), int(rng.integers(0, P.N.bit_length() - n_bits)))
    bits = b.unpack(rot[-1], int(rng.integers(1, 4)))
    packed = b.pack(b.pick(GL, int(rng.integers(1, 4)), among=vals))
    l0 += [b.op(FheOp.KeyswitchL1toL0, [x]) for x in bits[:2]]
    uni = b.op(TableOp.PBS_UNIVARIATE, [b.pick(L0, among=l0 + s[L0]), packed])
    biv = b.op(TableOp.PBS_BIVARIATE, [b.pick(L0, among=l0), b.pick(L0, among=s[L0] + [t[L0, 1]]), b.pick(GL, among=vals)],
               int(rng.choice((0, 63, int(rng.integers(1, 63))))))
    b.keep += [uni, biv, rot[-1], packed, glev, sel_ss, l0[-1]]
    if with_pufks:
        rows = l0 + s[L0] + [t[L0, 0]] if ValueKind(pufks_kind) == L0 else bits + s[L1] + [uni, biv, se, t[L1, 1]]
        k = b.pufks(b.pick(pufks_kind, int(rng.integers(1, 4)), among=rows))
        b.keep += [k, b.op(FheOp.CMux, [b.pick(GG, among=sels), k, b.pick(GL, among=vals)])]
    # two linear layers of either kind (W from 2 words to kN + 1 over the parameter sets): nine rows (above LWE_LINEAR_VT) over
    # five scattered operands, the first of them twice, then two rows over those nine in place
    kind = L0 if rng.random() < 0.5 else L1
    among = l0 + s[L0] + [t[L0, 0], t[L0, 1]] if kind == L0 else bits + s[L1] + [uni, biv, se, t[L1, 1]]
    ops = b.pick(kind, 4, among=among)
    first = b.linear(S_REPEAT, ops + [ops[0]])
    second = b.linear(S_SMALL, first)
    b.keep += [first[0], second[1]] + ([b.op(FheOp.KeyswitchL1toL0, [second[0]])] if kind == L1 else [])
    b.claim("linear_scattered_operand_repeated", lambda v: v.whole_group(first) and v.scattered(b.rec.inputs[first[0]]))
    b.claim("linear_in_place_over_a_previous_layer", lambda v: v.whole_group(second) and v.in_place(second[0]))
    if not b.glwe:
        return
    # a polynomial layer of five rows (above GLWE_POLY_VT) over seven scattered operands, the first of them twice, one row in place
    # over those five, and a node of each keyswitch mode over their rows: a drawn slot (either radix), a drawn round, the trace
    g = b.grng
    ops = [vals[int(a)] for a in g.integers(0, len(vals), size=6)]
    wide = b.poly_linear(P_WIDE, ops + [ops[0]])
    row = b.poly_linear(P_ROW, wide)
    new = [b.glwe_keyswitch(GLWE_KSK_TABLE[int(g.integers(0, 3))], row[0]), b.glwe_automorphism(int(g.integers(1, P.N.bit_length())), wide[1]),
           b.glwe_trace(wide[2])]
    b.keep += new + [wide[4]]
    b.claim("poly_scattered_operand_repeated", lambda v: v.whole_group(wide) and v.scattered(b.rec.inputs[wide[0]]))
    b.claim("poly_in_place_over_a_previous_layer", lambda v: v.whole_group(row) and v.in_place(row[0]))


def draw_circuit(seed, P, profile, pufks_kind=None, linear_seed=None, glwe=True, glwe_key_seed=None, glwe_poly_seed=None, glwe_other_radix=None):
    """-> (RecordedCircuit, facts).  facts: "patterns": the names of PATTERNS the circuit holds (claimed by the construction and
    confirmed on the planned levels); "refused": claimed but not confirmed; "pufks_kind": the operand kind
    of its public functional keyswitch nodes (drawn unless given; None without such nodes); "nodes" / "groups": counts by kind
    name; "linear_slots": the weight slots its linear nodes name, `draw_linear_slots(linear_seed)` (derived from `seed` unless
    given: circuits that share an engine or a group are drawn with one `linear_seed`), None for `pushable`.
    glwe: draw the polynomial linear maps and the GLWE keyswitch family too (GLWE_PATTERNS); without it the circuit is, node for
    node, what this generator drew before it knew them.  "glwe_ksk_slots": `draw_glwe_ksk_slots(glwe_key_seed, P, glwe_other_radix)`,
    "glwe_poly_slots": `draw_glwe_poly_slots(glwe_poly_seed, P.N)` (None for `pushable`); both seeds derived from `seed` unless given."""
    assert profile in PROFILES
    linear_seed = 0x11EA0000 + seed if linear_seed is None else linear_seed
    glwe_key_seed = 0x6B500000 + seed if glwe_key_seed is None else glwe_key_seed
    glwe_poly_seed = 0x61E00000 + seed if glwe_poly_seed is None else glwe_poly_seed
    b = _Builder(seed, P, profile)
    b.glwe = bool(glwe)
    with_pufks = profile != "pushable"
    if with_pufks and pufks_kind is None:
        pufks_kind = L0 if b.rng.random() < 0.7 else L1
    pufks_kind = ValueKind(pufks_kind) if with_pufks else None
    if profile == "small":
        _draw_small(b, with_pufks, pufks_kind)
    else:
        _draw_full(b, with_pufks, pufks_kind, _WIDTH_SETS[seed % 3])
    _outputs(b, 8 if profile == "small" else 30)
    v = _View(b.rec)
    held = {name for name, fn in b.claims if fn(v)}
    nodes, groups = {}, {}
    for i in range(len(b.rec.op)):
        name = kind_name(b.rec, i).split("(")[0]
        nodes[name] = nodes.get(name, 0) + 1
    for key, members in v.groups.items():
        name = kind_name(b.rec, members[0])
        groups[name] = groups.get(name, 0) + 1
    return b.rec, {"patterns": sorted(held), "refused": sorted({n for n, _ in b.claims} - held), "pufks_kind": pufks_kind,
                   "nodes": nodes, "groups": groups, "levels": max(v.level), "seed": seed, "profile": profile,
                   "linear_seed": linear_seed if with_pufks else None, "linear_slots": draw_linear_slots(linear_seed) if with_pufks else None,
                   "glwe_key_seed": glwe_key_seed if glwe else None, "glwe_poly_seed": glwe_poly_seed if glwe and with_pufks else None,
                   "glwe_ksk_slots": draw_glwe_ksk_slots(glwe_key_seed, P, glwe_other_radix) if glwe else None,
                   "glwe_poly_slots": draw_glwe_poly_slots(glwe_poly_seed, P.N) if glwe and with_pufks else None}
