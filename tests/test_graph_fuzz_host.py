"""The host side of the random differential tests of gate graphs (tests/test_gpu_graph_fuzz.py): the generator
(tests/graph_fuzz_cases.py) draws what it says it draws, and the model that is the GPU tests' only expectation
(tests/circuit_model.py) equals the compositions somebody wrote by hand for the kinds' own tests.  No device."""
import hashlib
import json
import os
import time

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, TableOp, ValueKind
from spf_amd import graph as G
from tests import blind_rotation_graph_cases as BR
from tests import circuit_model as M
from tests import glwe_keyswitch_cases as KC
from tests import glwe_keyswitch_graph_cases as GKG
from tests import glwe_poly_cases as GC
from tests import glwe_poly_graph_cases as GPG
from tests import graph_fuzz_cases as F
from tests import lwe_linear_cases as LC
from tests import lwe_linear_graph_cases as LG
from tests import pbs_graph_cases as K
from tests import pufks_cases as PC
from tests.polyref_cases import key_fft
from tests.util import random_glwe, random_lwe_batch

NODE_CONSTANTS = {name: getattr(G, name) for name in dir(G) if name.startswith("NODE_")}


def default_circuits(which, profile):
    """the circuits the GPU file draws on a context at the default count and seed"""
    P = K.keys_of(which)[0]
    test = {"full": 0, "pushable": 1}[profile]
    for case in range(F.DEFAULT_CASES):
        kind = F.tuned_pufks_kind(case) if which == "tuned" and profile == "full" else None
        yield F.draw_circuit(F.case_seed(F.DEFAULT_SEED, test, case), P, profile, kind)


def same_slots(a, b):
    """two weight-slot tables (or None twice) hold the same slots, weights and bias words"""
    if a is None or b is None:
        return a is None and b is None
    return a.keys() == b.keys() and all(np.array_equal(a[q][0], b[q][0]) and (a[q][1] is None) == (b[q][1] is None)
                                        and (a[q][1] is None or np.array_equal(a[q][1], b[q][1])) for q in a)


def same_ksk_slots(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.keys() == b.keys() and all(np.array_equal(a[q][0], b[q][0]) and a[q][1:] == b[q][1:] for q in a)


def same_poly_slots(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.keys() == b.keys() and all(all(np.array_equal(x, y) for x, y in zip(a[q][0], b[q][0])) and a[q][2] == b[q][2]
                                        and (a[q][1] is None) == (b[q][1] is None) and (a[q][1] is None or np.array_equal(a[q][1], b[q][1])) for q in a)


def circuit_digest(rec) -> str:
    """SHA-256 of everything a drawn circuit is: nodes, operands, parameters, outputs, the side tables and the inputs' words"""
    h = hashlib.sha256()
    h.update(json.dumps([rec.op, rec.kind, rec.param, [list(t) for t in rec.inputs], rec.outputs, sorted(rec._linear.items()),
                         sorted(rec._unpack_width.items())]).encode())
    for a in rec.host:
        if a is not None:
            h.update(np.ascontiguousarray(a).view(np.uint8).tobytes())
    return h.hexdigest()


def test_without_the_glwe_section_the_circuits_are_those_drawn_before_it():
    """tests/golden/graph_fuzz_circuits.json was recorded from the generator before it drew the polynomial linear maps and the GLWE
    keyswitch family, for the six drawn cases of tests/test_graph_plan.py's GOLDEN_CASES: `glwe=False` still draws them, node for
    node and word for word (their plans' digests in tests/golden/graph_plans.json say the same of the planner's view)"""
    from tests.test_graph_plan import GOLDEN_CASES
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_fuzz_circuits.json")) as f:
        golden = json.load(f)
    assert set(golden) == {name for name in GOLDEN_CASES if name.split("_")[0] in F.PROFILES} and len(golden) == 6
    for name, want in golden.items():
        rec = GOLDEN_CASES[name]()[0]
        assert not {G.NODE_GLWE_POLY_LINEAR, *F.GLWE_KS_KINDS} & set(rec.op), name
        assert (len(rec.op), len(rec.outputs), circuit_digest(rec)) == (want["nodes"], want["outputs"], want["sha256"]), name
        seed, profile = int(name.split("_")[1]), name.split("_")[0]
        with_glwe = F.draw_circuit(seed, {"tuned": K.keys_of("tuned")[0], "n128k2": K.TEST1, "n16k1": K.SMALL16}[name.split("_")[2]], profile)[0]
        assert len(with_glwe.op) > len(rec.op) and set(F.GLWE_KS_KINDS) <= set(with_glwe.op), name


def test_the_generator_is_deterministic():
    P = K.TEST1
    for profile in F.PROFILES:
        a, fa = F.draw_circuit(77, P, profile)
        b, fb = F.draw_circuit(77, P, profile)
        assert same_slots(fa.pop("linear_slots"), fb.pop("linear_slots"))     # (arrays: compared apart from the rest)
        assert same_ksk_slots(fa.pop("glwe_ksk_slots"), fb.pop("glwe_ksk_slots")) and same_poly_slots(fa.pop("glwe_poly_slots"), fb.pop("glwe_poly_slots"))
        assert (a.op, a.kind, a.param, a.inputs, a.outputs) == (b.op, b.kind, b.param, b.inputs, b.outputs) and fa == fb
        assert a._linear == b._linear
        assert all(x is None and y is None or np.array_equal(x, y) for x, y in zip(a.host, b.host))
        c, _ = F.draw_circuit(78, P, profile)
        assert (a.op, a.param, a.inputs) != (c.op, c.param, c.inputs)


@pytest.mark.parametrize("profile", F.PROFILES)
@pytest.mark.parametrize("which", K.CONTEXTS)
def test_every_circuit_is_one_recorded_circuit_accepts(which, profile):
    """replayed through RecordedCircuit's own checks (from_arrays calls every builder again); operands precede their users;
    the node and bootstrap budgets hold; a circuit has public functional keyswitch nodes of ONE operand kind, or none"""
    P = K.keys_of(which)[0]
    for seed in range(5):
        rec, facts = F.draw_circuit(seed, P, profile)
        assert all(j < i for i, ins in enumerate(rec.inputs) for j in ins)
        again = spf_amd.RecordedCircuit.from_arrays(rec.arrays(), rec.kind, rec.host, P.N)
        assert (again.op, again.kind, again.param, again.inputs) == (rec.op, rec.kind, rec.param, rec.inputs)
        assert again._linear == rec._linear and (profile == "pushable") == (not rec._linear)
        for i in rec._linear:                                  # every layer is of its slot's shape, and the slot is in the table
            if rec.op[i] == G.NODE_GLWE_POLY_LINEAR:
                assert (rec.linear_of(i)[1], len(rec.inputs[i])) == facts["glwe_poly_slots"][rec.linear_of(i)[0]][2]
                continue
            assert rec.linear_of(i) == (rec.linear_of(i)[0], facts["linear_slots"][rec.linear_of(i)[0]][0].shape[0])
            assert len(rec.inputs[i]) == facts["linear_slots"][rec.linear_of(i)[0]][0].shape[1]
        log_n = P.N.bit_length() - 1
        for i, op in enumerate(rec.op):                         # every slot a keyswitch node names is in the table, every round is one
            assert op != G.NODE_GLWE_KEYSWITCH or rec.param[i] in facts["glwe_ksk_slots"]
            assert op != G.NODE_GLWE_AUTOMORPHISM or 1 <= rec.param[i] <= log_n
        # the GLWE section is small work: layers of at most 9 rows, groups of the keyswitch family of at most 5
        assert max(rec.linear_of(i)[1] for i, op in enumerate(rec.op) if op == G.NODE_GLWE_POLY_LINEAR) <= 9 if profile != "pushable" else True
        groups = F.groups_of(rec, M.planned_levels(rec))
        assert max(len(m) for key, m in groups.items() if key[1] in F.GLWE_KS_KINDS) <= 5
        assert sorted(set(rec.outputs)) == again.outputs
        assert len(rec.op) <= (F.MAX_NODES_SMALL if profile == "small" else F.MAX_NODES), len(rec.op)
        for kind in ("CircuitBootstrap", "PBS_UNIVARIATE", "PBS_BIVARIATE"):
            assert 0 < facts["nodes"][kind] <= F.MAX_BOOTSTRAPS
        rows = {rec.kind[rec.inputs[i][0]] for i, op in enumerate(rec.op) if op == G.NODE_PUFKS}
        assert rows == (set() if profile == "pushable" else {int(facts["pufks_kind"])})
        assert all(rec.param[i] < P.N for i, op in enumerate(rec.op) if op in (int(FheOp.SampleExtract), G.NODE_UNPACK))
        if profile == "small":
            widths = [len(rec.inputs[i]) for i, op in enumerate(rec.op) if op in (G.NODE_PACK, G.NODE_PUFKS)]
            assert max(widths + list(rec._unpack_width.values())) <= 3


@pytest.mark.parametrize("which", K.CONTEXTS)
def test_the_default_seeds_reach_every_pattern_and_every_node_kind(which):
    """every name of PATTERNS is held (claimed by the construction AND confirmed on the planned levels) by a default circuit of
    each context, lowered and pushed; every FheOp, TableOp and NODE_* constant of spf_amd.graph is a node of every one"""
    assert len(NODE_CONSTANTS) >= 4 and len(list(FheOp)) + len(list(TableOp)) >= 12
    kinds = {int(op) for op in FheOp} | {int(op) for op in TableOp} | set(NODE_CONSTANTS.values())
    assert G.NODE_LWE_LINEAR == 68 and NODE_CONSTANTS["NODE_LWE_LINEAR"] == 68 and set(F.LINEAR_PATTERNS) <= set(F.PATTERNS)
    new_kinds = {"NODE_GLWE_POLY_LINEAR": 69, "NODE_GLWE_KEYSWITCH": 70, "NODE_GLWE_AUTOMORPHISM": 71, "NODE_GLWE_TRACE": 72}
    assert new_kinds.items() <= NODE_CONSTANTS.items() and set(F.GLWE_PATTERNS) <= set(F.PATTERNS) and len(NODE_CONSTANTS) >= 9
    assert set(F.GLWE_PUSHABLE_PATTERNS) < set(F.GLWE_KS_PATTERNS) and len(F.GLWE_PUSHABLE_PATTERNS) == len(F.GLWE_KS_PATTERNS) - 3
    glwe_left_out = set(F.GLWE_PATTERNS) - set(F.GLWE_PUSHABLE_PATTERNS)
    for profile, left_out in (("full", set()), ("pushable", set(F.PUFKS_PATTERNS) | set(F.LINEAR_PATTERNS) | glwe_left_out)):
        reached = set()
        for rec, facts in default_circuits(which, profile):
            reached |= set(facts["patterns"])
            # `pushable` lacks the kinds that have no submit by handle: of the four new ones, the polynomial linear map only
            missing = kinds - set(rec.op) - ({G.NODE_PUFKS, G.NODE_LWE_LINEAR, G.NODE_GLWE_POLY_LINEAR} if profile == "pushable" else set())
            assert not missing, (profile, facts["seed"], missing)
            assert (G.NODE_GLWE_POLY_LINEAR in rec.op) == (profile == "full")
            assert not (set(F.LINEAR_PATTERNS) | set(F.GLWE_PATTERNS)) & set(facts["refused"]), (profile, facts["seed"], facts["refused"])
            if profile == "full":                           # EVERY full circuit holds every linear layout, not one of the three
                assert set(F.LINEAR_PATTERNS) <= set(facts["patterns"]), (facts["seed"], sorted(set(F.LINEAR_PATTERNS) - set(facts["patterns"])))
            held = set(F.GLWE_PATTERNS) if profile == "full" else set(F.GLWE_PUSHABLE_PATTERNS)      # ... and every GLWE layout
            assert held <= set(facts["patterns"]), (profile, facts["seed"], sorted(held - set(facts["patterns"])))
            log_n = K.keys_of(which)[0].N.bit_length() - 1  # rounds 1 and log2 N in every circuit, the others drawn
            assert {1, log_n} <= {rec.param[i] for i, op in enumerate(rec.op) if op == G.NODE_GLWE_AUTOMORPHISM}
            assert {rec.param[i] for i, op in enumerate(rec.op) if op == G.NODE_GLWE_KEYSWITCH} == set(F.GLWE_KSK_TABLE)
            assert {-1, -2} <= set(rec.op)
        assert set(F.PATTERNS) - left_out <= reached, (profile, sorted(set(F.PATTERNS) - left_out - reached))
        assert reached <= set(F.PATTERNS)
    P = K.keys_of(which)[0]
    for seed in range(3):                   # the small profile: every kind, on any parameter set
        rec, facts = F.draw_circuit(seed, P, "small")
        assert kinds <= set(rec.op), kinds - set(rec.op)
        # its two layers: one above LWE_LINEAR_VT rows over scattered operands, one in place
        assert {"linear_scattered_operand_repeated", "linear_in_place_over_a_previous_layer"} <= set(facts["patterns"]), facts["refused"]
        assert max(rec.linear_of(i)[1] for i in rec._linear) > 8
        # its two polynomial layers: five rows (above GLWE_POLY_VT) over scattered operands, one row in place; one node per mode
        assert {"poly_scattered_operand_repeated", "poly_in_place_over_a_previous_layer"} <= set(facts["patterns"]), facts["refused"]
        assert not set(F.GLWE_PATTERNS) & set(facts["refused"])
        assert all(rec.op.count(kind) == 1 for kind in F.GLWE_KS_KINDS) and rec.op.count(G.NODE_GLWE_POLY_LINEAR) == 6


def test_planned_levels_on_a_graph_whose_levels_are_known():
    """the level passes of plan() on the shapes its comments name: a bootstrap with slack joins the one that must run soonest, a
    keyswitch head is pulled up against its first user"""
    rec = spf_amd.RecordedCircuit(16)
    x, l1, sel = rec.add_input(ValueKind.GLWE1, np.zeros(1)), rec.add_input(ValueKind.LWE1, np.zeros(1)), rec.add_input(ValueKind.GGSW1, np.zeros(1))
    ks = rec.add_op(FheOp.KeyswitchL1toL0, [l1])                        # ready at 1, first user at 4: pulled to 3
    a = rec.add_op(FheOp.Not, [rec.add_op(FheOp.Not, [rec.add_op(FheOp.CMux, [sel, x, x])])])     # levels 1, 2, 3
    late = rec.add_op(FheOp.CircuitBootstrap, [rec.add_op(FheOp.KeyswitchL1toL0, [rec.add_op(FheOp.SampleExtract, [a], 0)])])   # 4, 5, 6
    early = rec.add_op(FheOp.CircuitBootstrap, [ks])                    # ready at 2, needed at 7: runs with `late` at 6
    rec.add_op(FheOp.CMux, [early, rec.add_op(FheOp.CMux, [late, a, x]), x])
    assert M.planned_levels(rec) == [0, 0, 0, 5, 1, 2, 3, 4, 5, 6, 6, 7, 8]


# ---- the model against compositions written by hand ---------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["n128k2", "n16k1"])
def test_the_model_equals_oracle_shift_right(which):
    P, ks, ak, ssk = K.keys_of(which)
    s_bits, x_bits = 2, 3
    x, s = random_glwe(0xF00, 2, P.glwe_len)
    rec = spf_amd.RecordedCircuit(P.N)
    BR.shift_right_graph(rec, rec.add_input(ValueKind.GLWE1, x), rec.add_input(ValueKind.GLWE1, s), s_bits, x_bits)
    vals = M.evaluate(rec, P, M.keys_of(which))
    rotated, lwes = BR.oracle_shift_right(P, ks, ak, ssk, x, s, s_bits, x_bits)
    assert K.same_words(vals[rec.outputs[0]], rotated)
    for node, want in zip(rec.outputs[1:], lwes):
        assert K.same_words(vals[node], want)


def test_the_model_equals_oracle_loop_on_a_rotation_graph():
    P = K.TEST1
    glwes, sels = random_glwe(0xF10, 2, P.glwe_len), BR.random_selectors(0xF11, 3, P)

    class Eng:                      # rotation_graph reads the degree off its engine; the circuit it fills is given
        params = K.engine_params(P)

    rec, _ = BR.rotation_graph(Eng, glwes, sels, 2, circuit=spf_amd.RecordedCircuit(P.N))
    vals = M.evaluate(rec, P, M.keys_of("n128k2"))
    for node, x in zip(rec.outputs, glwes):
        assert K.same_words(vals[node], BR.oracle_loop(x, sels, 2, P))


def test_the_model_equals_pufks_oracle_on_a_keyswitch_node():
    P = K.TEST1
    log, count = 4, 3
    key = K.pufks_key(P.N, P.k, P.lwe_n, count)
    rows = random_lwe_batch(0xF20, 4, P.lwe_n)
    rec = spf_amd.RecordedCircuit(P.N)
    ids = [rec.add_input(ValueKind.LWE0, r) for r in rows]
    node = rec.add_public_functional_keyswitch([ids[i] for i in (2, 0, 3, 3, 1)])
    vals = M.evaluate(rec, P, M.keys_of("n128k2", (key, log, count)))
    assert K.same_words(vals[node], PC.pufks_oracle(rows[[2, 0, 3, 3, 1]], key_fft(key), P.N, P.k, log, count).reshape(-1))


def test_draw_linear_slots_is_deterministic_and_holds_every_class_shape_and_bias_state():
    slots, again, other = F.draw_linear_slots(11), F.draw_linear_slots(11), F.draw_linear_slots(12)
    assert same_slots(slots, again) and set(slots) == {q for q, *_ in F.LINEAR_SLOTS} == set(other)
    assert all(0 <= q < G.LWE_LINEAR_SLOTS for q in slots) and G.LWE_LINEAR_SLOTS - 1 in slots
    shapes = {q: w.shape for q, (w, _) in slots.items()}
    assert shapes == F.LINEAR_SHAPE == {q: other[q][0].shape for q in other}          # a fixed table: only the contents are drawn
    assert all(not np.array_equal(slots[q][0], other[q][0]) for q in slots if slots[q][0].size > 4)
    assert {M for M, _ in shapes.values()} >= {1, 8, 9, 17} and any(1 < M < 8 for M, _ in shapes.values())      # around LWE_LINEAR_VT
    assert {Kk for _, Kk in shapes.values()} >= {1, 4, 8} and any(Kk % 4 for _, Kk in shapes.values() if Kk > 1)  # the unroll
    assert shapes[F.S_A] == shapes[F.S_B] and not np.array_equal(slots[F.S_A][0], slots[F.S_B][0])
    assert {b is None for _, b in slots.values()} == {True, False}
    classes = {q: LC.limbs_of(int(w.min()), int(w.max())) for q, (w, _) in slots.items()}
    assert {1, 2, 3, 0} <= set(classes.values())
    for q, M, Kk, cls, bias in F.LINEAR_SLOTS:
        w, b = slots[q]
        assert w.dtype == np.int64 and (b is None) == (not bias) and (b is None or (b.dtype == np.uint64 and b.shape == (M,)))
        assert classes[q] == (cls if cls in (1, 2, 3) else 0), q
        if cls == "beyond":
            assert (w == LC.FIRST_BEYOND[1]).any()
        if cls == "int64":
            assert all((w == v).any() for v in (LC.INT64_MIN, -1, 0, LC.INT64_MAX)), q
    given, derived, next_ = (F.draw_circuit(seed, K.TEST1, "full", linear_seed=ls)[1] for seed, ls in ((3, 11), (3, None), (4, None)))
    assert given["linear_seed"] == 11 and same_slots(given["linear_slots"], slots)
    assert len({11, derived["linear_seed"], next_["linear_seed"]}) == 3           # derived from the circuit seed unless given
    assert same_slots(derived["linear_slots"], F.draw_linear_slots(derived["linear_seed"]))


@pytest.mark.parametrize("slot", [q for q, *_ in F.LINEAR_SLOTS])
def test_the_model_equals_linear_literal_on_a_linear_node(slot):
    """the reference's loop on Python integers (independent of `linear_ref`), for a slot of each weight class, shape and bias
    state; operands of both kinds with a repeat among them"""
    P = K.TEST1
    w, b = F.draw_linear_slots(0xF40)[slot]
    rows_out, Kk = w.shape
    for kind, dim in ((ValueKind.LWE0, P.lwe_n), (ValueKind.LWE1, P.k * P.N)):
        rows = random_lwe_batch(0xF41 + slot, Kk, dim)
        rec = spf_amd.RecordedCircuit(P.N)
        ids = [rec.add_input(kind, r) for r in rows]
        order = [(3 * j + 1) % Kk for j in range(Kk - 1)] + [0]               # a permutation for odd K, repeats elsewhere
        nodes = rec.add_lwe_linear(slot, [ids[j] for j in order], rows_out)
        vals = M.evaluate(rec, P, M.Keys(None, None, None, None, {slot: (w, b)}))      # (no key but the weight slots)
        want = LC.linear_literal(rows[order], w, b)
        for m, node in enumerate(nodes):
            assert K.same_words(vals[node], np.array(want[m], dtype=np.uint64)), (slot, kind, m)


@pytest.mark.parametrize("kind", [ValueKind.LWE0, ValueKind.LWE1], ids=["lwe0", "lwe1"])
def test_the_model_equals_chain_by_oracle_on_the_recorded_chain(kind):
    """tests/lwe_linear_graph_cases.py's "layer -> table -> layer -> table", recorded: the walk its own GPU test compares with"""
    which = "n16k1"
    P, ks = K.keys_of(which)[:2]
    Kk, M1, M2 = 4, 3, 2
    (wa, ba), (wb, bb) = LG.weights(0xF50, M1, Kk, True), LG.weights(0xF51, M2, M1, False)
    luts = random_glwe(0xF52, 2, P.glwe_len)
    x = LC.uniform_inputs(0xF53, 1, Kk, LG.words(P, kind))[0]

    class Rec(spf_amd.RecordedCircuit):     # chain() keeps what add_output returns: here the node, not an array to be filled
        def add_output(self, node, kind):
            super().add_output(node, kind)
            return node

    rec = Rec(P.N)
    outs = LG.chain(rec, kind, 20, 21, x, luts[0], luts[1], M1, M2)
    vals = M.evaluate(rec, P, M.keys_of(which, None, {20: (wa, ba), 21: (wb, bb)}))
    want = LG.chain_by_oracle(P, ks, kind, x, wa, ba, wb, bb, luts[0], luts[1])
    for name in ("a", "h", "b", "y"):
        assert K.same_words(np.stack([vals[n] for n in outs[name]]), want[name]), name


@pytest.mark.parametrize("which", K.CONTEXTS)
def test_the_model_equals_the_expressions_of_the_computed_table_test(which):
    """test_gpu_pbs_graph.py::test_a_computed_table_and_operands_from_two_levels: the same graph, recorded"""
    P, ks, ak, ssk = K.keys_of(which)
    x0, l1, lut = random_lwe_batch(0xE10, 1, P.lwe_n)[0], random_lwe_batch(0xE11, 1, P.k * P.N)[0], random_glwe(0xE12, 1, P.glwe_len)[0]
    g = spf_amd.RecordedCircuit(P.N)
    t = g.add_op(FheOp.MulXN, [g.add_input(ValueKind.GLWE1, lut)], 5)
    a = g.add_input(ValueKind.LWE0, x0)
    b = g.add_op(FheOp.KeyswitchL1toL0, [g.add_input(ValueKind.LWE1, l1)])
    uni = [g.add_op(FheOp.PBS_UNIVARIATE, [n, t]) for n in (b, a)]
    biv = g.add_op(FheOp.PBS_BIVARIATE, [b, a, t], 1)
    vals = M.evaluate(g, P, M.keys_of(which))
    t_want = O.glwe_mul_xn(lut, 5, P.N, P.k)
    b_want = O.keyswitch_lwe(l1, ks.ksk, P.k * P.N, P.lwe_n, P.ks_radix_log, P.ks_count)
    assert K.same_words(vals[uni[0]], O.pbs_univariate(b_want, t_want, ks.bsk_fft, P))
    assert K.same_words(vals[uni[1]], O.pbs_univariate(x0, t_want, ks.bsk_fft, P))
    assert K.same_words(vals[biv], O.pbs_univariate(K.pack(b_want, x0, 1), t_want, ks.bsk_fft, P))


def test_the_model_states_the_constants_and_the_keyless_kinds_as_their_tests_do():
    """test_gpu_graph.py::test_graph_ggsw_and_glev_constants and test_gpu_values.py:98-108, at (N, k) = (128, 2)"""
    P, ks, ak, ssk = K.keys_of("n128k2")
    a, b = random_glwe(0xF30, 2, P.glwe_len)
    ga, gb = random_glwe(0xF31, 2, P.cbs_count * P.glwe_len)
    ggsw = BR.random_selectors(0xF32, 1, P)[0]
    rec = spf_amd.RecordedCircuit(P.N)
    na, nb = rec.add_input(ValueKind.GLWE1, a), rec.add_input(ValueKind.GLWE1, b)
    nga, ngb, ng = rec.add_input(ValueKind.GLEV1, ga), rec.add_input(ValueKind.GLEV1, gb), rec.add_input(ValueKind.GGSW1, ggsw)
    one = rec.add_trivial(ValueKind.GGSW1, 1)
    nodes = {"mul": rec.add_op(FheOp.MultiplyGgswGlwe, [ng, na]), "gc": rec.add_op(FheOp.GlevCMux, [ng, nga, ngb]),
             "ss": rec.add_op(FheOp.SchemeSwitch, [rec.add_trivial(ValueKind.GLEV1, 1)]), "cmux": rec.add_op(FheOp.CMux, [ng, na, nb]),
             "pack": rec.add_pack([na, nb, na]), "xn": rec.add_op(FheOp.MulXN, [na], 2 * P.N + 77)}
    vals = M.evaluate(rec, P, M.keys_of("n128k2"))
    cb = (P.N, P.k, P.cbs_radix_log, P.cbs_count)
    triv = np.zeros(P.lwe_n + 1, dtype=np.uint64)
    triv[-1] = np.uint64(1 << 63)
    assert K.same_words(vals[one], O.circuit_bootstrap(triv, ks.bsk_fft, ak, ssk, P))
    glev = np.zeros((P.cbs_count, P.k + 1, P.N), dtype=np.uint64)
    for j in range(P.cbs_count):
        glev[j, P.k, 0] = np.uint64(1 << (64 - P.cbs_radix_log * (j + 1)))
    assert K.same_words(vals[nodes["ss"]], O.scheme_switch_fft(glev.reshape(-1), ssk, P))
    h = P.N // 2
    fft = O.glwe_ggsw_mad(np.zeros((P.k + 1) * h, dtype=np.complex128), a, ggsw, *cb)
    assert K.same_words(vals[nodes["mul"]], np.concatenate([O.poly_ifft(fft[q * h:(q + 1) * h]) for q in range(P.k + 1)]))
    for j in range(P.cbs_count):
        want = O.cmux(ga.reshape(P.cbs_count, -1)[j], gb.reshape(P.cbs_count, -1)[j], ggsw, *cb)
        assert K.same_words(vals[nodes["gc"]].reshape(P.cbs_count, -1)[j], want)
    assert K.same_words(vals[nodes["cmux"]], O.cmux(a, b, ggsw, *cb))
    assert K.same_words(vals[nodes["xn"]], O.glwe_mul_xn(a, 77, P.N, P.k))
    want = a + O.glwe_mul_xn(b, 1, P.N, P.k) + O.glwe_mul_xn(a, 2, P.N, P.k)
    assert K.same_words(vals[nodes["pack"]], want)


# ---- the polynomial linear maps and the GLWE keyswitch family -----------------------------------------------------------------------

def test_draw_glwe_ksk_slots_is_deterministic_and_holds_both_radices():
    for P in (K.keys_of("tuned")[0], K.TEST1, K.SMALL16):
        slots, again, other = F.draw_glwe_ksk_slots(11, P), F.draw_glwe_ksk_slots(11, P), F.draw_glwe_ksk_slots(12, P)
        assert same_ksk_slots(slots, again) and set(slots) == set(F.GLWE_KSK_TABLE) == set(other)
        assert {0, G.GLWE_KSK_SLOTS - 1} <= set(slots) and all(0 <= q < G.GLWE_KSK_SLOTS for q in slots)
        trace = (P.tr_radix_log, P.tr_count)
        assert slots[F.K_A][1:] == slots[F.K_B][1:] == trace and not np.array_equal(slots[F.K_A][0], slots[F.K_B][0])
        assert slots[F.K_OTHER][1:] != trace and slots[F.K_OTHER][1:] == F.other_radix_of(P)
        for q, (words, lg, cnt) in slots.items():
            assert words.dtype == np.uint64 and words.shape == (P.k, cnt, P.k + 1, P.N) and lg * cnt <= 64
            assert other[q][1:] == (lg, cnt) and not np.array_equal(other[q][0], words)       # only the contents are drawn
        assert F.draw_glwe_ksk_slots(11, P, (3, 5))[F.K_OTHER][1:] == (3, 5)
    assert F.other_radix_of(K.keys_of("tuned")[0]) == KC.OTHER_RADIX      # the generic kernel inside a tuned graph
    given, derived, next_ = (F.draw_circuit(seed, K.TEST1, "pushable", glwe_key_seed=ks)[1] for seed, ks in ((3, 11), (3, None), (4, None)))
    assert given["glwe_key_seed"] == 11 and same_ksk_slots(given["glwe_ksk_slots"], F.draw_glwe_ksk_slots(11, K.TEST1))
    assert len({11, derived["glwe_key_seed"], next_["glwe_key_seed"]}) == 3 and given["glwe_poly_slots"] is None


@pytest.mark.parametrize("N", [16, 128, 2048])
def test_draw_glwe_poly_slots_is_deterministic_and_holds_every_class_shape_and_bias_state(N):
    slots, again, other = F.draw_glwe_poly_slots(11, N), F.draw_glwe_poly_slots(11, N), F.draw_glwe_poly_slots(12, N)
    assert same_poly_slots(slots, again) and set(slots) == {q for q, *_ in F.GLWE_POLY_TABLE} == set(other)
    assert all(0 <= q < G.GLWE_POLY_SLOTS for q in slots) and G.GLWE_POLY_SLOTS - 1 in slots
    shapes = {q: shape for q, (_, _, shape) in slots.items()}
    assert shapes == F.GLWE_POLY_SHAPE == {q: other[q][2] for q in other} and set(shapes.values()) == set(GPG.SCATTERED_SHAPES)
    assert {m for m, _ in shapes.values()} >= {1, GPG.VT, GPG.VT + 1, 9} and {k % 4 for _, k in shapes.values()} >= {0, 1, 2, 3}
    assert shapes[F.P_A] == shapes[F.P_B] and F.GLWE_POLY_CLASS[F.P_A] != F.GLWE_POLY_CLASS[F.P_B]
    assert sum(b is not None for _, b, _ in slots.values()) == sum(b is None for _, b, _ in slots.values()) == len(slots) // 2
    seams = GC.seam_exponents(N)
    for q, M_, K_, cls, bias in F.GLWE_POLY_TABLE:
        (off, exp, coef), b, shape = slots[q]
        assert shape == (M_, K_) and len(off) == M_ * K_ + 1 and (b is None) == (not bias) and (b is None or b.shape == (M_, N))
        assert GC.is_constants_only((off, exp, coef)) == (cls != "general")
        if cls == "empty":
            assert len(exp) == 0 and b is not None
            continue
        first = slice(int(off[0]), int(off[1]))                 # polynomial (0, 0): every extreme coefficient, every seam exponent
        assert set(GC.EXTREME_COEFFICIENTS) <= set(coef[first].tolist())
        assert set(exp[first].tolist()) >= (set(seams) if cls == "general" else {0})
        assert set(exp.tolist()) <= set(seams) and int(exp.max(initial=0)) < N
        assert not np.array_equal(coef, other[q][0][2])
    derived = F.draw_circuit(3, K.TEST1, "full")[1]
    assert same_poly_slots(derived["glwe_poly_slots"], F.draw_glwe_poly_slots(derived["glwe_poly_seed"], K.TEST1.N))
    assert same_poly_slots(F.draw_circuit(3, K.TEST1, "full", glwe_poly_seed=11)[1]["glwe_poly_slots"], F.draw_glwe_poly_slots(11, K.TEST1.N))


class _Recorded(spf_amd.RecordedCircuit):
    """a recording in the place of an FheCircuit: add_output gives the node back, where a graph gives the array it fills"""

    def add_output(self, node, kind):
        super().add_output(node, kind)
        return node


def _keys_of_case(c, poly=None):
    """the model's keys for a case of glwe_keyswitch_cases: its automorphism key and the slots `glwe_keyswitch_graph_cases.load_keys` fills"""
    ksk = {slot: (words, lg, cnt) for slot, (words, _, (lg, cnt)) in GKG.slot_keys(c).items()}
    N = c.P.N
    return M.Keys(None, c.ak_fft, None, None, None, ksk, poly or {GKG.XINV_SLOT: (GKG.xinv(N), None, (1, 1)), GKG.TWO_TERM_SLOT: (GKG.two_terms(N), None, (1, 1))})


@pytest.mark.parametrize("mode", range(3), ids=["keyswitch", "automorphism", "trace"])
@pytest.mark.parametrize("shape", ["N16", GKG.TUNED])
def test_the_model_equals_the_scattered_graph_of_the_keyswitch_family(monkeypatch, shape, mode):
    """glwe_keyswitch_graph_cases.Scattered at B = 5, recorded: `Scattered.check` compares the model's words with the expectation
    the GPU tests of the three nodes use (the oracle on the operand nodes' own words)"""
    c = KC.case(shape)
    name, kind, param = GKG.modes(c)[mode]
    monkeypatch.setattr(spf_amd, "FheCircuit", lambda eng: _Recorded(c.P.N))
    s = GKG.Scattered(None, c, 0xF60, kind, param, 5)
    rec = s.g
    assert rec.op.count(kind) == 10 and G.NODE_GLWE_POLY_LINEAR in rec.op
    vals = M.evaluate(rec, c.P, _keys_of_case(c))
    s.producers, s.over_inputs, s.over_level1 = ([vals[n] for n in nodes] for nodes in (s.producers, s.over_inputs, s.over_level1))
    s.check(f"the model, {name}")
    if shape == GKG.TUNED and mode == 0:        # the other-radix slot: the key's own radix, not the context's
        s = GKG.Scattered(None, c, 0xF61, kind, GKG.OTHER_SLOT, 5)
        vals = M.evaluate(s.g, c.P, _keys_of_case(c))
        s.producers, s.over_inputs, s.over_level1 = ([vals[n] for n in nodes] for nodes in (s.producers, s.over_inputs, s.over_level1))
        s.check("the model, keyswitch under the other radix")


@pytest.mark.parametrize("shape", ["N16", GKG.TUNED])
def test_the_model_equals_xinv_then_trace_then_sample_extract(shape):
    """the chain of test_gpu_glwe_keyswitch_graph.py::test_xinv_then_trace_then_sample_extract_isolates_one_coefficient, recorded,
    against that test's expectations; the trace node also against `oracle_fold`, the rounds one by one"""
    c = KC.case(shape)
    P = c.P
    ones = KC.all_ones_glwe(c)
    rec = spf_amd.RecordedCircuit(P.N)
    x = rec.add_input(ValueKind.GLWE1, ones)
    shifted = rec.add_glwe_poly_linear(GKG.XINV_SLOT, [x], 1)[0]
    traced = rec.add_glwe_trace(shifted)
    se = rec.add_op(FheOp.SampleExtract, [traced], 0)
    switched = rec.add_glwe_keyswitch(GKG.A2B_SLOT, x)
    rounds = [rec.add_glwe_automorphism(r, x) for r in range(1, KC.log2n(P) + 1)]
    vals = M.evaluate(rec, P, _keys_of_case(c))
    want_shifted = GKG.poly_row(c, GKG.xinv(P.N), ones)
    want_traced = GKG.oracle_trace(c, want_shifted)
    assert GKG.same_words(vals[shifted], want_shifted) and GKG.same_words(vals[traced], want_traced)
    assert GKG.same_words(vals[se], O.sample_extract(want_traced.reshape(-1), 0, P.N, P.k))
    KC.check_can_trace(c, vals[traced], "model")
    assert GKG.same_words(vals[switched], KC.oracle_keyswitch(P, ones, c.ksk_fft))
    assert GKG.same_words(vals[traced], KC.oracle_fold(c, want_shifted))
    for r, node in enumerate(rounds, 1):
        assert GKG.same_words(vals[node], KC.oracle_round(c, ones, r)), r
        assert GKG.same_words(M.oracle_round(P, c.ak_fft.reshape(-1), ones, r), KC.oracle_round(c, ones, r)), r


@pytest.mark.parametrize("which", ["n128k2", "n16k1"])
def test_the_model_equals_the_pool_graph_of_the_polynomial_layers(monkeypatch, which):
    """glwe_poly_graph_cases.pool_graph at (M, K) = (5, 7), recorded, for every slot variant of that module: the nodes around by
    `GlwePool.by_oracle`, the layers by `poly_linear_ref` on the operand nodes' own words, as the GPU test compares"""
    P = K.keys_of(which)[0]
    k1, N = GPG.dims(P)
    Mr, Kk = 5, 7
    monkeypatch.setattr(spf_amd, "FheCircuit", lambda eng: _Recorded(N))
    rec, pool, pk, outs = GPG.pool_graph(None, P, 3, GPG.LAYERS, Kk, Mr, 0xF70)
    for name, (triple, bias) in GPG.slots(Mr, Kk, N).items():
        vals = M.evaluate(rec, P, M.Keys(None, None, None, None, None, None, {3: (triple, bias, (Mr, Kk))}))
        nodes = np.stack([vals[n] for n in pool.outs])
        assert K.same_words(nodes, pool.by_oracle()), name
        rows = np.stack([np.stack([nodes[i] for i in p]) for p in pk]).reshape(GPG.LAYERS, Kk, k1, N)
        got = np.stack([np.stack([vals[n] for n in layer]) for layer in outs]).reshape(GPG.LAYERS, Mr, k1, N)
        assert K.same_words(got, GC.poly_linear_ref(rows, triple, Mr, Kk, bias)), name


# ---- the comparison -------------------------------------------------------------------------------------------------------------

def test_the_comparison_bites():
    """one word of one input changed: every output the model computes from that input differs under `same_words`, the others do
    not, and `first_difference` names the lowest of them.  One of the inputs reaches the outputs through linear layers only, and
    one through polynomial layers and the GLWE keyswitch family only"""
    which = "n16k1"
    P = K.keys_of(which)[0]
    rec, facts = F.draw_circuit(5, P, "full", ValueKind.LWE0)
    keys = M.keys_of(which, (K.pufks_key(P.N, P.k, P.lwe_n, 3), 4, 3), facts["linear_slots"], facts["glwe_ksk_slots"], facts["glwe_poly_slots"])
    users = [[i for i, ins in enumerate(rec.inputs) if node in ins] for node in range(len(rec.op))]
    only_linear = [node for node, op in enumerate(rec.op) if op == -1 and users[node] and all(rec.op[u] == G.NODE_LWE_LINEAR for u in users[node])]
    new_kinds = (G.NODE_GLWE_POLY_LINEAR,) + F.GLWE_KS_KINDS
    only_glwe = [node for node, op in enumerate(rec.op) if op == -1 and users[node] and all(rec.op[u] in new_kinds for u in users[node])]
    assert only_linear and only_glwe and {rec.op[u] for node in only_glwe for u in users[node]} == set(new_kinds)
    only_linear += only_glwe
    want = M.evaluate(rec, P, keys)
    assert M.first_difference(rec, [want[n] for n in rec.outputs], want) is None
    depends = [set() for _ in rec.op]
    for i, ins in enumerate(rec.inputs):
        depends[i] = {i}.union(*[depends[j] for j in ins])
    flipped = 0
    for node in [i for i, op in enumerate(rec.op) if op == -1]:
        if not any(node in depends[o] for o in rec.outputs):
            continue
        host = rec.host[node].view(np.uint64).reshape(-1).copy()
        host[host.size // 2] ^= np.uint64(1 << 63)
        got = M.evaluate(rec, P, keys, hosts={node: host})
        hit = [o for o in rec.outputs if node in depends[o] and not K.same_words(got[o], want[o])]
        assert hit, node                                    # (a CMUX rounds: not every dependent word has to move, some must)
        assert all(K.same_words(got[o], want[o]) for o in rec.outputs if node not in depends[o])
        message = M.first_difference(rec, [got[n] for n in rec.outputs], want)
        assert message is not None and f"lowest node {min(hit)} " in message, message
        flipped += 1
        if node in only_linear:
            only_linear.remove(node)
    assert flipped >= 10 and not only_linear


def test_time_of_the_model_on_a_full_circuit_of_the_tuned_set():
    """sizes the GPU tests' node budget (profiles/r23_graph_fuzz.md, r29_graph_fuzz_linear.md): the oracle walks a default
    circuit in seconds"""
    P = K.keys_of("tuned")[0]
    rec, facts = F.draw_circuit(F.case_seed(F.DEFAULT_SEED, 0, 0), P, "full", ValueKind.LWE0)
    keys = M.keys_of("tuned", (K.pufks_key(P.N, P.k, P.lwe_n, 8, seed=4), 4, 8), facts["linear_slots"], facts["glwe_ksk_slots"], facts["glwe_poly_slots"])
    t0 = time.perf_counter()
    vals = M.evaluate(rec, P, keys)
    seconds = time.perf_counter() - t0
    print(f"model: {len(rec.op)} nodes of the tuned set in {seconds:.2f} s")
    assert len(vals) == len(rec.op) and seconds < 20
