"""The plaintext linear maps over LWE ciphertexts as gate-graph nodes (`spf_graph_add_lwe_linear`, include/spf_hip.h), on the
tuned DEFAULT_128 kernels (W1 = 2049 words, a short LWE side: W0 = 13) and on generic contexts at (N, k) = (128, 2) and (16, 1)
(W1 = 257 and 17): the body word alone in a last column block, and a whole row inside one partial block.  Every comparison is on
words (tests/lwe_linear_graph_cases.py): against `linear_ref` on the operand nodes' own words — every operand node is an output
too — against `Engine.lwe_linear` on the same rows, and against the oracle for the nodes around the linear node.  One case
decrypts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import spf_amd
from spf_amd import FheOp, ValueKind
from tests import lwe_linear_cases as LC
from tests import lwe_linear_graph_cases as G
from tests.util import random_glwe, random_lwe_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(which):
        if which not in made:
            made[which] = G.make_engine(which)
        return G.keys_of(which)[0], made[which], G.keys_of(which)[1]

    yield get
    for e in made.values():
        e.close()


def kind_id(kind):
    return ValueKind(kind).name.lower()


# ---- 1. scattered operands ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kind", G.KINDS, ids=kind_id)
@pytest.mark.parametrize("M,K", G.SCATTERED_SHAPES)
@pytest.mark.parametrize("which", G.CONTEXTS)
def test_scattered_operands_take_one_launch_of_the_rows_kernel(rigs, which, M, K, kind, bias):
    P, eng, ks = rigs(which)
    G.load_pool_key(eng, which, P, kind)
    w, b = G.weights(0xEC00 + 16 * M + K, M, K, bias)
    eng.load_lwe_linear_weights(3, w, b)
    assert eng.lwe_linear_slot_shape(3) == (M, K, bias)
    g, rows_of, outs = G.pool_graph(eng, P, kind, 3, G.LAYERS, K, M, 0xEC10 + K)
    g.run()
    assert eng.last_lwe_linear_kernel() == G.ROWS_KERNEL
    g.close()
    rows, got = rows_of(), G.stack(outs)
    assert rows.shape == (G.LAYERS, K, G.words(P, kind)) and got.shape == (G.LAYERS, M, G.words(P, kind))
    assert G.same_words(got, LC.linear_ref(rows, w, b)), (M, K)
    assert G.same_words(got, eng.lwe_linear(3, rows, int(kind))), (M, K)


# ---- 2. in-place operands -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", G.CONTEXTS)
def test_in_place_operands_go_to_the_batch_dispatcher(rigs, which):
    P, eng, ks = rigs(which)
    layers, K, M1, M2 = 2, 4, 9, 3
    wa, ba = G.weights(0xEC20, M1, K, True)
    wb, bb = G.weights(0xEC21, M2, M1, False)
    eng.load_lwe_linear_weights(6, wa, ba)
    eng.load_lwe_linear_weights(7, wb, bb)
    # set A: the K operands of every layer are results of ONE keyswitch group, in its order
    l1 = random_lwe_batch(0xEC22, layers * K, P.k * P.N)
    g = spf_amd.FheCircuit(eng)
    l0 = [g.add_op(FheOp.KeyswitchL1toL0, [g.add_input(ValueKind.LWE1, v)]) for v in l1]
    row_outs = [g.add_output(n, ValueKind.LWE0) for n in l0]
    a = [g.add_lwe_linear(6, l0[q * K:(q + 1) * K]) for q in range(layers)]
    a_outs = [[g.add_output(n, ValueKind.LWE0) for n in layer] for layer in a]
    g.run()
    assert eng.last_lwe_linear_kernel() in G.BATCH_KERNELS and eng.last_lwe_linear_kernel() != G.ROWS_KERNEL
    # gather of the inputs, keyswitch, ONE launch for both layers (the VALU product at this size)
    assert g.stats() == {"nodes": 2 * layers * K + layers * M1, "levels": 2, "launches": 3}, g.stats()
    g.close()
    rows = np.stack(row_outs).reshape(layers, K, P.lwe_n + 1)
    assert G.same_words(rows.reshape(layers * K, -1), eng.keyswitch_lwe_l1_lwe_l0(l1))
    assert G.same_words(G.stack(a_outs), LC.linear_ref(rows, wa, ba))
    assert G.same_words(G.stack(a_outs), eng.lwe_linear(6, rows, int(ValueKind.LWE0)))
    # set B: the K operands are the M results of a previous linear node (itself over scattered inputs)
    for kind in G.KINDS:
        W = G.words(P, kind)
        x = LC.uniform_inputs(0xEC23, 1, K, W)[0]
        g = spf_amd.FheCircuit(eng)
        xs, _ = G.input_rows(g, kind, x)
        first = g.add_lwe_linear(6, xs)
        second = g.add_lwe_linear(7, first)
        outs = [[g.add_output(n, kind) for n in layer] for layer in (first, second)]
        g.run()
        assert eng.last_lwe_linear_kernel() in G.BATCH_KERNELS
        assert g.stats() == {"nodes": K + M1 + M2, "levels": 2, "launches": 2}, g.stats()
        g.close()
        mid = LC.linear_ref(x, wa, ba)
        assert G.same_words(np.stack(outs[0]), mid), kind
        assert G.same_words(np.stack(outs[1]), LC.linear_ref(mid, wb, bb)), kind
        assert G.same_words(np.stack(outs[1]), eng.lwe_linear(7, np.stack(outs[0])[None], int(kind))[0]), kind


# ---- 3. grouping --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", G.CONTEXTS)
def test_layers_of_one_slot_kind_and_level_are_one_launch(rigs, which):
    P, eng, ks = rigs(which)
    M, K = 3, 2
    w0, b0 = G.weights(0xEC30, M, K, True)
    w1, _ = G.weights(0xEC31, M, K, False)
    eng.load_lwe_linear_weights(10, w0, b0)
    eng.load_lwe_linear_weights(11, w1)
    x0 = LC.uniform_inputs(0xEC32, 3, K, P.lwe_n + 1)
    x1 = LC.uniform_inputs(0xEC33, 1, K, P.k * P.N + 1)

    def graph(plan):
        """plan: [(slot, kind, layer index)] -> (stats, [(M, W) words per entry])"""
        g = spf_amd.FheCircuit(eng)
        ins0 = [G.input_rows(g, ValueKind.LWE0, x)[0] for x in x0]
        ins1 = [G.input_rows(g, ValueKind.LWE1, x)[0] for x in x1]
        outs = []
        for slot, kind, q in plan:
            ids = (ins0 if kind == ValueKind.LWE0 else ins1)[q]
            outs.append([g.add_output(n, kind) for n in g.add_lwe_linear(slot, ids)])
        g.run()
        st = g.stats()
        g.close()
        return st, [np.stack(o) for o in outs]

    base, _ = graph([])
    L0, L1 = ValueKind.LWE0, ValueKind.LWE1
    st, got = graph([(10, L0, 0), (10, L0, 1), (10, L0, 2)])
    assert st == {"nodes": base["nodes"] + 3 * M, "levels": 1, "launches": base["launches"] + 1}, (st, base)
    for q in range(3):
        assert G.same_words(got[q], LC.linear_ref(x0[q], w0, b0)), q
    assert not np.array_equal(got[2], got[0])
    st, got = graph([(10, L0, 0), (11, L0, 1)])                       # two slots on one level
    assert st["launches"] == base["launches"] + 2 and st["levels"] == 1, st
    assert G.same_words(got[0], LC.linear_ref(x0[0], w0, b0)) and G.same_words(got[1], LC.linear_ref(x0[1], w1))
    st, got = graph([(10, L0, 0), (10, L1, 0)])                       # one slot, both kinds
    assert st["launches"] == base["launches"] + 2 and st["levels"] == 1, st
    assert G.same_words(got[0], LC.linear_ref(x0[0], w0, b0)) and G.same_words(got[1], LC.linear_ref(x1[0], w0, b0))


# ---- 4. weights the limbs cannot hold -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", G.KINDS, ids=kind_id)
@pytest.mark.parametrize("which", G.CONTEXTS)
def test_weights_beyond_three_limbs_on_the_scattered_path(rigs, which, kind):
    P, eng, ks = rigs(which)
    G.load_pool_key(eng, which, P, kind)
    M, K = G.HARD_WEIGHTS.shape
    bias = np.array([LC.M64, 1 << 63, 0], dtype=np.uint64)
    eng.load_lwe_linear_weights(12, G.HARD_WEIGHTS, bias)
    g, rows_of, outs = G.pool_graph(eng, P, kind, 12, 2, K, M, 0xEC40)
    g.run()
    assert eng.last_lwe_linear_kernel() == G.ROWS_KERNEL
    g.close()
    assert G.same_words(G.stack(outs), LC.linear_ref(rows_of(), G.HARD_WEIGHTS, bias))


# ---- 5. the chain ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", G.KINDS, ids=kind_id)
@pytest.mark.parametrize("which", G.CONTEXTS)
def test_layer_table_layer_table_in_one_run_twice(rigs, which, kind):
    P, eng, ks = rigs(which)
    K, M1, M2, W = 4, 3, 2, G.words(P, kind)
    wa, ba = G.weights(0xEC50, M1, K, True)
    wb, bb = G.weights(0xEC51, M2, M1, False)
    eng.load_lwe_linear_weights(20, wa, ba)
    eng.load_lwe_linear_weights(21, wb, bb)
    luts = random_glwe(0xEC52, 2, P.glwe_len)
    xs = LC.uniform_inputs(0xEC53, 2, K, W)
    x = xs[0].copy()
    g = spf_amd.FheCircuit(eng)
    outs = G.chain(g, kind, 20, 21, x, luts[0], luts[1], M1, M2)
    for run in range(2):
        x[...] = xs[run]                                    # the second run: new contents of the inputs, the same graph
        g.run()
        want = G.chain_by_oracle(P, ks, kind, xs[run], wa, ba, wb, bb, luts[0], luts[1])
        for name in ("a", "h", "b", "y"):
            assert G.same_words(np.stack(outs[name]), want[name]), (run, name)
    st = g.stats()
    # layer A | (keyswitch |) table 1 | layer B | keyswitch | table 2
    assert st["nodes"] == 2 + K + (3 if kind == ValueKind.LWE1 else 2) * M1 + 3 * M2, st
    assert st["levels"] == (6 if kind == ValueKind.LWE1 else 5), st
    assert eng.last_lwe_linear_kernel() in G.BATCH_KERNELS  # layer B reads the bootstrap group's results in place
    g.close()


def test_the_chain_decrypts_to_the_plaintext_model(rigs):
    P, eng, ks = rigs("tuned")
    lut1, lut2 = G.model_tables(P)
    eng.load_lwe_linear_weights(22, G.MODEL_WA, G.model_bias_words())
    eng.load_lwe_linear_weights(23, G.MODEL_WB)
    x = G.model_encrypt(ks, 0)
    g = spf_amd.FheCircuit(eng)
    outs = G.chain(g, ValueKind.LWE0, 22, 23, x, lut1, lut2, 3, 2)
    for run in range(2):
        x[...] = G.model_encrypt(ks, run)
        g.run()
        assert G.model_decrypt(ks, outs["y"]) == G.model(G.MODEL_INPUTS[run]), run
    g.close()


# ---- 6. reload ------------------------------------------------------------------------------------------------------------------

def test_a_slot_loaded_again_between_runs_gives_the_new_weights(rigs):
    P, eng, ks = rigs("n128k2")
    G.reload_rounds(eng, P)


def test_a_reload_after_the_capture_drops_the_replayed_graph():
    """SPF_GRAPH_CAPTURE=1 is read once per process, hence the child: the second run captures, the third replays, the slots are
    loaded again (their old images are freed), the fourth run must give the new weights' words"""
    code = ("import spf_amd\n"
            "from tests import lwe_linear_graph_cases as G\n"
            "P = G.keys_of('n128k2')[0]\n"
            "eng = spf_amd.Engine(G.engine_params(P))\n"
            "G.reload_rounds(eng, P)\n"
            "eng.close()\nprint('reload ok')\n")
    env = dict(os.environ, SPF_GRAPH_CAPTURE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, env=env, timeout=300)
    assert r.returncode == 0 and "reload ok" in r.stdout, r.stderr[-3000:]


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_the_graph_stays_usable(rigs):
    P, eng, ks = rigs("tuned")
    w, b = G.weights(0xEC70, 2, 2, True)
    eng.load_lwe_linear_weights(30, w, b)
    x0, x1 = random_lwe_batch(0xEC71, 2, P.lwe_n), random_lwe_batch(0xEC72, 1, P.k * P.N)[0]
    g = spf_amd.FheCircuit(eng)
    a, a2 = (g.add_input(ValueKind.LWE0, v) for v in x0)
    l1 = g.add_input(ValueKind.LWE1, x1)
    lut = g.add_input(ValueKind.GLWE1, random_glwe(0xEC73, 1, P.glwe_len)[0])
    lib, n_nodes = eng._lib, g.stats()["nodes"]
    out = (C.c_uint32 * (G.MAX_ROWS + 1))(*([77] * (G.MAX_ROWS + 1)))
    add = lib.spf_graph_add_lwe_linear

    def refused(status_call, word):
        assert status_call() == 1
        assert word in lib.spf_last_error(eng._h).decode(), lib.spf_last_error(eng._h)
        assert g.stats()["nodes"] == n_nodes and set(out) == {77}       # nothing recorded

    two = (C.c_uint32 * 2)(a, a2)
    refused(lambda: add(g._g, G.SLOTS, two, 2, 2, out), "slot")
    refused(lambda: add(g._g, 30, two, 0, 2, out), "K")
    refused(lambda: add(g._g, 30, two, 2, 0, out), "M")
    refused(lambda: add(g._g, 30, two, 2, G.MAX_ROWS + 1, out), "M")
    refused(lambda: add(g._g, 30, None, 2, 2, out), "null")
    refused(lambda: add(g._g, 30, two, 2, 2, None), "null")
    refused(lambda: add(g._g, 30, (C.c_uint32 * 2)(a, n_nodes), 2, 2, out), "not a node")
    refused(lambda: add(g._g, 30, (C.c_uint32 * 2)(a, lut), 2, 2, out), "not an LWE")
    refused(lambda: add(g._g, 30, (C.c_uint32 * 2)(a, l1), 2, 2, out), "mixed")
    refused(lambda: add(g._g, 30, (C.c_uint32 * 2)(l1, a), 2, 2, out), "mixed")
    assert add(None, 30, two, 2, 2, out) == 1
    with pytest.raises(spf_amd.SpfError, match="K = 0"):
        g.add_lwe_linear(30, [])
    with pytest.raises(spf_amd.SpfError) as e:
        g.add_lwe_linear(31, [a, a2])                                    # M=None asks the engine: the slot is empty
    assert e.value.status == G.NO_KEY and g.stats()["nodes"] == n_nodes
    rows = g.add_lwe_linear(30, [a2, a])                                 # ... and the graph still runs
    assert rows == [n_nodes, n_nodes + 1]
    outs = [g.add_output(n, ValueKind.LWE0) for n in rows]
    g.run()
    assert G.same_words(np.stack(outs), LC.linear_ref(x0[::-1], w, b))
    assert g.add_lwe_linear(30, [a] * 3, G.MAX_ROWS) == list(range(n_nodes + 2, n_nodes + 2 + G.MAX_ROWS))   # M at the limit: accepted
    g.close()


def test_errors_of_the_run_and_the_graph_still_runs_once_the_weights_are_there():
    P = G.keys_of("n16k1")[0]
    eng = spf_amd.Engine(G.engine_params(P))
    try:
        x = LC.uniform_inputs(0xEC80, 1, 5, P.lwe_n + 1)[0]
        g = spf_amd.FheCircuit(eng)
        xs, _ = G.input_rows(g, ValueKind.LWE0, x)
        outs = [g.add_output(n, ValueKind.LWE0) for n in g.add_lwe_linear(40, xs, 3)]   # built before the slot is loaded
        with pytest.raises(spf_amd.SpfError) as e:
            g.run()
        assert e.value.status == G.NO_KEY and "slot 40" in str(e.value), str(e.value)
        eng.load_lwe_linear_weights(40, *G.weights(0xEC81, 7, 6, True))
        with pytest.raises(spf_amd.SpfError) as e:
            g.run()
        assert e.value.status == 1 and all(f" {v} " in f" {e.value} " for v in (7, 6, 3, 5)), str(e.value)
        w, b = G.weights(0xEC82, 3, 5, True)
        eng.load_lwe_linear_weights(40, w, b)
        g.run()
        assert G.same_words(np.stack(outs), LC.linear_ref(x, w, b))
        g.close()
    finally:
        eng.close()


# ---- 8. group, 9. recorded circuit ------------------------------------------------------------------------------------------------

def two_layer_job(g, kind, x, slot_a, slot_b, M1=None, M2=None):
    xs = [g.add_input(kind, row) for row in x]
    a = g.add_lwe_linear(slot_a, xs[::-1], M1)
    b = g.add_lwe_linear(slot_b, a, M2)
    return [g.add_output(n, kind) for n in a + b]


def test_group_jobs_carry_linear_nodes_through_a_merge(rigs):
    """two jobs over members [0, 0] — whichever way they are dealt, the words are those of the graphs run alone"""
    P, eng, ks = rigs("n128k2")
    K, M1, M2 = 3, 9, 2
    wa, ba = G.weights(0xEC90, M1, K, True)
    wb, bb = G.weights(0xEC91, M2, M1, True)
    xs = {ValueKind.LWE0: LC.uniform_inputs(0xEC92, 1, K, P.lwe_n + 1)[0], ValueKind.LWE1: LC.uniform_inputs(0xEC93, 1, K, P.k * P.N + 1)[0]}
    eng.load_lwe_linear_weights(50, wa, ba)
    eng.load_lwe_linear_weights(51, wb, bb)
    alone = {}
    for kind, x in xs.items():
        g = spf_amd.FheCircuit(eng)
        outs = two_layer_job(g, kind, x, 50, 51)
        g.run()
        g.close()
        alone[kind] = np.stack(outs)
        mid = LC.linear_ref(x[::-1], wa, ba)
        assert G.same_words(alone[kind], np.concatenate([mid, LC.linear_ref(mid, wb, bb)]))
    grp = spf_amd.Group(G.engine_params(P), devices=[0, 0])
    jobs = []
    try:
        grp.load_lwe_linear_weights(50, wa, ba)
        grp.load_lwe_linear_weights(51, wb, bb)
        assert grp.lwe_linear_slot_shape(51) == (M2, M1, True)
        for kind, x in xs.items():
            g = spf_amd.FheCircuit(grp)
            jobs.append((g, kind, two_layer_job(g, kind, x, 50, 51)))   # (M=None: the group is asked for the slots' shapes)
        grp.run_graphs([g for g, _, _ in jobs])
        for _, kind, outs in jobs:
            assert G.same_words(np.stack(outs), alone[kind]), kind
    finally:
        for g, _, _ in jobs:
            g.close()
        grp.close()


def test_recorded_circuit_lowers_to_the_same_words(rigs):
    P, eng, ks = rigs("n16k1")
    K, M1, M2 = 3, 2, 9
    eng.load_lwe_linear_weights(60, *G.weights(0xECA0, M1, K, True))
    eng.load_lwe_linear_weights(61, *G.weights(0xECA1, M2, M1, False))
    x = LC.uniform_inputs(0xECA2, 1, K, P.k * P.N + 1)[0]
    g = spf_amd.FheCircuit(eng)
    direct = two_layer_job(g, ValueKind.LWE1, x, 60, 61)
    g.run()
    g.close()
    rec = spf_amd.RecordedCircuit(P.N)
    two_layer_job(rec, ValueKind.LWE1, x, 60, 61, M1, M2)
    h, outs = rec.lower(eng)
    h.run()
    assert h.stats()["nodes"] == K + M1 + M2
    h.close()
    assert G.same_words(np.stack(outs), np.stack(direct))
    again = spf_amd.RecordedCircuit.from_arrays(rec.arrays(), rec.kind, rec.host, P.N)
    assert again.op == rec.op and again.param == rec.param and again.inputs == rec.inputs and again._linear == rec._linear
