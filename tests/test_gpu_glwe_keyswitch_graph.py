"""The GLWE keyswitch, one automorphism round and the homomorphic trace as gate-graph nodes (`spf_graph_add_glwe_keyswitch`,
`spf_graph_add_glwe_automorphism`, `spf_graph_add_glwe_trace`, include/spf_hip.h) on the tuned DEFAULT_128 kernels, on generic
contexts at (N, k) = (256, 3) and (16, 1), and under a key of another radix on the tuned context.  Every node is an output, so
every word the new nodes write is compared (tests/glwe_keyswitch_graph_cases.py): against the oracle's `keyswitch_glwe_to_glwe`,
round and `trace` on the operand nodes' own words.  There is no tolerance in this file; the two decryption checks use the
reference's decode at 12 plaintext bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import glwe_keyswitch_cases as KC
from tests import glwe_keyswitch_graph_cases as G
from tests.blind_rotation_graph_cases import random_selectors
from tests.util import random_lwe_batch

pytestmark = pytest.mark.gpu
GLWE = ValueKind.GLWE1
U = np.uint64
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)


@pytest.fixture(scope="module")
def rigs():
    """one context per shape with every key of G.load_keys, made when a test first asks for it"""
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = G.make_engine(shape)
        return KC.case(shape), made[shape]

    yield get
    for e in made.values():
        e.close()


def run_stats(g):
    g.run()
    return g.stats()


def drawn(shapes=G.SHAPES, other=True):
    """(shape, mode name, kind, param) of every case: the three modes on every shape, and the other-radix slot on the tuned one"""
    out = []
    for shape in shapes:
        for name, kind, param in G.modes():
            out.append(pytest.param(shape, kind, param, id=f"{shape}-{name}"))
    if other:
        out.append(pytest.param(G.TUNED, G.KS, G.OTHER_SLOT, id=f"{G.TUNED}-keyswitch-other-radix"))
    return out


def batches(shape, kind, param, rows):
    """B of a group: G.BATCHES, B = 2 under the other-radix key; a rows kernel needs two operands (one alone lies consecutively)"""
    bs = (2,) if param == G.OTHER_SLOT and kind == G.KS else G.BATCHES[shape]
    return [b for b in bs if b > 1] if rows else bs


# ---- 1. scattered operands -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,kind,param", drawn())
def test_scattered_operands_take_one_launch_of_a_rows_kernel(rigs, shape, kind, param):
    c, eng = rigs(shape)
    base = G.Scattered(eng, c, 0xB10)
    base_stats = run_stats(base.g)
    base.g.close()
    for B in batches(shape, kind, param, rows=True):
        s = G.Scattered(eng, c, 0xB10, kind, param, B)
        st = run_stats(s.g)
        assert eng.last_glwe_keyswitch_kernel() == G.ROWS[G.is_tuned(c, kind, param)], (shape, B)
        # the B nodes over the inputs and the B nodes over level 1 are ONE launch each, whatever B
        assert st == {"nodes": base_stats["nodes"] + 2 * B, "levels": 2, "launches": base_stats["launches"] + 2}, (st, base_stats)
        s.check((shape, kind, param, B))
        s.g.close()


# ---- 2. consecutive operands -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,kind,param", drawn())
def test_consecutive_operands_go_to_the_in_place_kernels(rigs, shape, kind, param):
    c, eng = rigs(shape)
    P = c.P
    for B in batches(shape, kind, param, rows=False):
        def graph(with_nodes):
            g = spf_amd.FheCircuit(eng)
            ins = [g.add_input(GLWE, v) for v in c.x]
            xs = [g.add_op(FheOp.GlweAdd, [ins[j], ins[(j + 1) % KC.ITEMS]]) for j in range(B)]   # ONE group: consecutive rows
            rows = [g.add_output(n, GLWE) for n in xs]
            return g, rows, [g.add_output(G.add_node(g, kind, param, n), GLWE) for n in xs] if with_nodes else []

        g, _, _ = graph(False)
        base = run_stats(g)
        g.close()
        g, rows, outs = graph(True)
        st = run_stats(g)
        assert eng.last_glwe_keyswitch_kernel() == G.IN_PLACE[G.is_tuned(c, kind, param)], (shape, B)
        assert st == {"nodes": base["nodes"] + B, "levels": 2, "launches": base["launches"] + 1}, (st, base)
        g.close()
        for j in range(B):
            assert G.same_words(rows[j], O.glwe_xor(c.x[j].reshape(-1), c.x[(j + 1) % KC.ITEMS].reshape(-1), P.N, P.k)), (shape, B, j)
            assert G.same_words(outs[j], G.oracle_node(c, kind, param, rows[j])), (shape, B, j)


# ---- 3. consumers ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", G.SHAPES)
def test_every_kind_of_consumer_reads_a_nodes_row(rigs, shape):
    """the row of a node of each mode as the source of a SampleExtract and of an unpack, the low and the high operand of a CMUX,
    the operand of a polynomial linear map and of a second keyswitch under another slot: each against the oracle walking the
    node's own output words"""
    c, eng = rigs(shape)
    P = c.P
    sel = random_selectors(0xB30, 1, P)[0]
    g = spf_amd.FheCircuit(eng)
    ins = [g.add_input(GLWE, v) for v in c.x[:2]]
    s = g.add_input(ValueKind.GGSW1, sel)
    got = []
    for name, kind, param in G.modes(c):
        n = G.add_node(g, kind, param, ins[0])
        got.append(dict(row=g.add_output(n, GLWE),
                        ext=g.add_output(g.add_op(FheOp.SampleExtract, [n], P.N - 1), ValueKind.LWE1),
                        bits=[g.add_output(b, ValueKind.LWE1) for b in g.add_unpack(n, 3)],
                        low=g.add_output(g.add_op(FheOp.CMux, [s, n, ins[1]]), GLWE),
                        high=g.add_output(g.add_op(FheOp.CMux, [s, ins[1], n]), GLWE),
                        poly=g.add_output(g.add_glwe_poly_linear(G.XINV_SLOT, [n], 1)[0], GLWE),
                        again=g.add_output(g.add_glwe_keyswitch(G.SECOND_SLOT, n), GLWE)))
    g.run()
    g.close()
    for (name, kind, param), o in zip(G.modes(c), got):
        row = o["row"]
        assert G.same_words(row, G.oracle_node(c, kind, param, c.x[0])), (shape, name)
        assert G.same_words(o["ext"], O.sample_extract(row, P.N - 1, P.N, P.k)), (shape, name)
        for j in range(3):
            assert G.same_words(o["bits"][j], O.sample_extract(row, j, P.N, P.k)), (shape, name, j)
        assert G.same_words(o["low"], G.cmux(c, row, c.x[1], sel)), (shape, name)
        assert G.same_words(o["high"], G.cmux(c, c.x[1], row, sel)), (shape, name)
        assert G.same_words(o["poly"], G.poly_row(c, G.xinv(P.N), row)), (shape, name)
        assert G.same_words(o["again"], G.oracle_node(c, G.KS, G.SECOND_SLOT, row)), (shape, name)


# ---- 4. grouping -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [G.TUNED, "N16"])
def test_nodes_of_one_mode_and_parameter_are_one_launch(rigs, shape):
    c, eng = rigs(shape)

    def graph(plan):
        """plan: [(kind, param, which input)] -> (stats, output arrays)"""
        g = spf_amd.FheCircuit(eng)
        ins = [g.add_input(GLWE, v) for v in c.x]
        outs = [g.add_output(G.add_node(g, kind, param, ins[i]), GLWE) for kind, param, i in plan]
        st = run_stats(g)
        g.close()
        return st, outs

    def check(plan, launches):
        st, outs = graph(plan)
        assert st == {"nodes": KC.ITEMS + len(plan), "levels": 1, "launches": launches}, (plan, st)
        for (kind, param, i), got in zip(plan, outs):
            assert G.same_words(got, G.oracle_node(c, kind, param, c.x[i])), (shape, kind, param, i)

    check([(G.KS, G.A2B_SLOT, 3), (G.KS, G.A2B_SLOT, 0)], 1)                 # one slot: one group
    check([(G.KS, G.A2B_SLOT, 3), (G.KS, G.SECOND_SLOT, 0)], 2)              # two slots: two
    check([(G.AU, 1, 4), (G.AU, 1, 1), (G.AU, 1, 2)], 1)                     # one round: one group
    check([(G.AU, 1, 4), (G.AU, KC.log2n(c.P), 1)], 2)                       # two rounds: two
    check([(G.TR, 0, 2), (G.TR, 0, 0), (G.KS, G.A2B_SLOT, 0), (G.AU, 2, 0)], 3)   # the three modes: one each


# ---- 5. a composition under real keys -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [G.TUNED, "N16"])
def test_xinv_then_trace_then_sample_extract_isolates_one_coefficient(rigs, shape):
    """X^-j, trace, SampleExtract(0) inside ONE run: the all-ones polynomial at 12 plaintext bits keeps its coefficient j, N-fold,
    in coefficient 0 and nothing elsewhere (`can_trace`, ops/automorphisms/mod.rs:101-136); a keyswitch to the second secret key in
    the same run keeps the phase"""
    c, eng = rigs(shape)
    P = c.P
    ones = KC.all_ones_glwe(c)
    g = spf_amd.FheCircuit(eng)
    x = g.add_input(GLWE, ones)
    shifted = g.add_glwe_poly_linear(G.XINV_SLOT, [x], 1)[0]
    traced = g.add_glwe_trace(shifted)
    outs = [g.add_output(n, k) for n, k in ((shifted, GLWE), (traced, GLWE), (g.add_op(FheOp.SampleExtract, [traced], 0), ValueKind.LWE1),
                                            (g.add_glwe_keyswitch(G.A2B_SLOT, x), GLWE))]
    st = run_stats(g)
    assert st == {"nodes": 5, "levels": 3, "launches": 4}, st
    g.close()
    want_shifted = G.poly_row(c, G.xinv(P.N), ones)
    want_traced = G.oracle_trace(c, want_shifted)
    assert G.same_words(outs[0], want_shifted) and G.same_words(outs[1], want_traced)
    assert G.same_words(outs[2], O.sample_extract(want_traced.reshape(-1), 0, P.N, P.k))
    KC.check_can_trace(c, outs[1], "graph")
    assert G.same_words(outs[3], KC.oracle_keyswitch(P, ones, c.ksk_fft))
    KC.check_switched_phase(c, ones[None], G.glwe(c, outs[3])[None], "graph")


# ---- 6. the keys at run time ------------------------------------------------------------------------------------------------------

def test_errors_of_the_run_and_the_graph_still_runs_once_the_key_is_there():
    c = KC.case("N16")
    P = c.P
    eng = spf_amd.Engine(G.engine_params(P))
    try:
        g = spf_amd.FheCircuit(eng)
        ins = [g.add_input(GLWE, v) for v in c.x]
        switched = [g.add_glwe_keyswitch(G.EMPTY_SLOT, ins[i]) for i in (4, 1, 4)]     # built before any key is loaded
        outs = [g.add_output(n, GLWE) for n in switched]
        for o in outs:
            o[...] = SENTINEL
        with pytest.raises(spf_amd.SpfError) as e:
            g.run()
        assert e.value.status == G.NO_KEY and f"slot {G.EMPTY_SLOT}" in str(e.value), str(e.value)
        assert all((o == SENTINEL).all() for o in outs), "a refused run wrote an output"
        traced = g.add_output(g.add_glwe_trace(switched[0]), GLWE)
        traced[...] = SENTINEL
        eng.load_glwe_keyswitch_key_std(G.EMPTY_SLOT, c.ksk, P.tr_radix_log, P.tr_count)
        with pytest.raises(spf_amd.SpfError) as e:
            g.run()                                                        # the slot is there, the automorphism key is not
        assert e.value.status == G.NO_KEY and "automorphism key" in str(e.value), str(e.value)
        assert all((o == SENTINEL).all() for o in outs + [traced]), "a refused run wrote an output"
        eng.load_automorphism_key_std(np.ascontiguousarray(c.hk.ak))
        g.run()
        assert eng.last_glwe_keyswitch_kernel() == G.IN_PLACE[False]       # (the trace of one row)
        for i, o in zip((4, 1, 4), outs):
            assert G.same_words(o, KC.oracle_keyswitch(P, c.x[i], c.ksk_fft)), i
        assert G.same_words(traced, G.oracle_trace(c, outs[0]))
        g.close()
    finally:
        eng.close()


@pytest.mark.parametrize("shape", [G.TUNED, "N16"])
def test_a_slot_loaded_again_between_runs_gives_the_new_keys_words(rigs, shape):
    c, eng = rigs(shape)
    G.reload_rounds(eng, c)


def test_a_reload_to_another_radix_changes_the_kernel(rigs):
    """the slot's device buffer AND the kernel that serves it change under a graph that is already planned"""
    c, eng = rigs(G.TUNED)
    P = c.P
    words, fft = KC.other_radix_key(c, seed=2)
    eng.load_glwe_keyswitch_key_std(8, c.ksk, P.tr_radix_log, P.tr_count)
    g = spf_amd.FheCircuit(eng)
    ins = [g.add_input(GLWE, v) for v in c.x]
    outs = [g.add_output(g.add_glwe_keyswitch(8, ins[i]), GLWE) for i in (2, 0)]
    g.run()
    assert eng.last_glwe_keyswitch_kernel() == G.ROWS[True]
    for i, o in zip((2, 0), outs):
        assert G.same_words(o, KC.oracle_keyswitch(P, c.x[i], c.ksk_fft)), i
    eng.load_glwe_keyswitch_key_std(8, words, *KC.OTHER_RADIX)
    g.run()
    assert eng.last_glwe_keyswitch_kernel() == G.ROWS[False]
    for i, o in zip((2, 0), outs):
        assert G.same_words(o, KC.oracle_keyswitch(P, c.x[i], fft, KC.OTHER_RADIX)), i
    g.close()


def test_a_reload_after_the_capture_drops_the_replayed_graph():
    """SPF_GRAPH_CAPTURE=1 is read once per process, hence the child: the second run captures, the third replays, the slot is
    loaded again (its old buffer is freed), the fourth run must give the new key's words"""
    code = ("import spf_amd\n"
            "from tests import glwe_keyswitch_cases as KC\n"
            "from tests import glwe_keyswitch_graph_cases as G\n"
            "c = KC.case('N16')\n"
            "eng = spf_amd.Engine(G.engine_params(c.P))\n"
            "G.reload_rounds(eng, c)\n"
            "eng.close()\nprint('reload ok')\n")
    env = dict(os.environ, SPF_GRAPH_CAPTURE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, env=env, timeout=300)
    assert r.returncode == 0 and "reload ok" in r.stdout, r.stderr[-3000:]


# ---- 7. bad arguments ------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_the_graph_stays_usable(rigs):
    c, eng = rigs(G.TUNED)
    P = c.P
    log_n = KC.log2n(P)
    g = spf_amd.FheCircuit(eng)
    a = g.add_input(GLWE, c.x[0])
    l1 = g.add_input(ValueKind.LWE1, random_lwe_batch(0xB70, 1, P.k * P.N)[0])
    glev = g.add_trivial(ValueKind.GLEV1, 1)
    l0 = g.add_input(ValueKind.LWE0, random_lwe_batch(0xB71, 1, P.lwe_n)[0])
    lib, n_nodes = eng._lib, g.stats()["nodes"]
    out = C.c_uint32(77)
    ks, au, tr = lib.spf_graph_add_glwe_keyswitch, lib.spf_graph_add_glwe_automorphism, lib.spf_graph_add_glwe_trace

    def refused(status_call, prefix, *words):
        assert status_call() == G.INVALID
        message = lib.spf_last_error(eng._h).decode()
        assert message.startswith(prefix) and all(w in message for w in words), message
        assert g.stats()["nodes"] == n_nodes and out.value == 77        # nothing recorded, node_out untouched

    for slot in (16, 17, 0xFFFFFFFF):
        refused(lambda: ks(g._g, slot, a, C.byref(out)), "graph GLWE keyswitch: ", f"slot {slot} >= SPF_GLWE_KSK_SLOTS = 16")
    for rnd in (0, log_n + 1, 0xFFFFFFFF):
        refused(lambda: au(g._g, rnd, a, C.byref(out)), "graph GLWE automorphism: ", f"round {rnd} outside 1 .. log2 N = {log_n}")
    refused(lambda: ks(g._g, 0, a, None), "graph GLWE keyswitch: ", "null pointer")
    refused(lambda: au(g._g, 1, a, None), "graph GLWE automorphism: ", "null pointer")
    refused(lambda: tr(g._g, a, None), "graph GLWE trace: ", "null pointer")
    for bad, kind in ((l1, int(ValueKind.LWE1)), (glev, int(ValueKind.GLEV1)), (l0, int(ValueKind.LWE0))):
        refused(lambda: ks(g._g, 0, bad, C.byref(out)), "graph GLWE keyswitch: ", f"operand {bad} is not an L1 GLWE", f"kind is {kind}")
        refused(lambda: au(g._g, 1, bad, C.byref(out)), "graph GLWE automorphism: ", f"operand {bad} is not an L1 GLWE")
        refused(lambda: tr(g._g, bad, C.byref(out)), "graph GLWE trace: ", f"operand {bad} is not an L1 GLWE")
    for bad in (n_nodes, 0xFFFFFFFF):
        refused(lambda: ks(g._g, 0, bad, C.byref(out)), "graph GLWE keyswitch: ", f"operand {bad} is not a node of this graph", f"{n_nodes} nodes")
        refused(lambda: tr(g._g, bad, C.byref(out)), "graph GLWE trace: ", f"operand {bad} is not a node of this graph")
    assert ks(None, 0, a, C.byref(out)) == G.INVALID and au(None, 1, a, C.byref(out)) == G.INVALID and tr(None, a, C.byref(out)) == G.INVALID
    assert out.value == 77
    with pytest.raises(spf_amd.SpfError, match="slot must be in 0 .. 15"):
        g.add_glwe_keyswitch(16, a)
    with pytest.raises(spf_amd.SpfError, match="outside 1 .. log2 N"):
        g.add_glwe_automorphism(0, a)
    # ... and the graph still takes nodes and runs: the limits themselves are accepted
    nodes = [g.add_glwe_keyswitch(15, a), g.add_glwe_automorphism(log_n, a), g.add_glwe_automorphism(1, a), g.add_glwe_trace(a)]
    assert nodes == list(range(n_nodes, n_nodes + 4))
    eng.load_glwe_keyswitch_key_std(15, c.ksk, P.tr_radix_log, P.tr_count)
    outs = [g.add_output(n, GLWE) for n in nodes]
    g.run()
    g.close()
    for o, (kind, param) in zip(outs, ((G.KS, G.A2B_SLOT), (G.AU, log_n), (G.AU, 1), (G.TR, 0))):   # (slot 15 holds slot A2B's key)
        assert G.same_words(o, G.oracle_node(c, kind, param, c.x[0])), (kind, param)


# ---- 8. group jobs, a recorded circuit ---------------------------------------------------------------------------------------------

def chain_job(g, c, picks):
    """keyswitch, round 2 and trace over the inputs `picks` (scattered), then the trace of every keyswitched row (in place) and a
    keyswitch of every trace under the second slot -> output arrays, node-major"""
    ins = [g.add_input(GLWE, c.x[i]) for i in range(KC.ITEMS)]
    outs = []
    first = [[G.add_node(g, kind, param, ins[i]) for i in picks] for _, kind, param in G.modes(c)]
    second = [g.add_glwe_trace(n) for n in first[0]]
    third = [g.add_glwe_keyswitch(G.SECOND_SLOT, n) for n in second]
    for n in first[0] + first[1] + first[2] + second + third:
        outs.append(g.add_output(n, GLWE))
    return outs


def chain_by_oracle(c, picks):
    first = [[G.oracle_node(c, kind, param, c.x[i]) for i in picks] for _, kind, param in G.modes(c)]
    second = [G.oracle_trace(c, r) for r in first[0]]
    third = [G.oracle_node(c, G.KS, G.SECOND_SLOT, r) for r in second]
    return first[0] + first[1] + first[2] + second + third


def test_group_jobs_carry_the_nodes_through_a_merge(rigs):
    """two jobs with the same nodes over members [0, 0] — whichever way they are dealt, the words are those of the graphs run
    alone on one context, which are the oracle's"""
    c, eng = rigs("N16")
    all_picks = ([4, 0, 4], [1, 3, 2])
    alone = []
    for picks in all_picks:
        g = spf_amd.FheCircuit(eng)
        outs = chain_job(g, c, picks)
        st = run_stats(g)
        assert st["levels"] == 3 and st["launches"] == 5, st               # three modes | the traces | the second keyswitches
        g.close()
        for j, (got, want) in enumerate(zip(outs, chain_by_oracle(c, picks))):
            assert G.same_words(got, want), (picks, j)
        alone.append(np.stack(outs))
    grp = spf_amd.Group(G.engine_params(c.P), devices=[0, 0])
    jobs = []
    try:
        g = spf_amd.FheCircuit(grp)
        jobs.append((g, chain_job(g, c, all_picks[0])))                    # built before the group's keys are loaded
        with pytest.raises(spf_amd.SpfError) as e:
            grp.run_graphs([g])                                            # the merged graph checks the member's keys
        assert e.value.status == G.NO_KEY
        G.load_keys(grp, c)
        g = spf_amd.FheCircuit(grp)
        jobs.append((g, chain_job(g, c, all_picks[1])))
        grp.run_graphs([g for g, _ in jobs])
        for j, (_, outs) in enumerate(jobs):
            assert G.same_words(np.stack(outs), alone[j]), j
    finally:
        for g, _ in jobs:
            g.close()
        grp.close()


def test_recorded_circuit_lowers_to_the_same_words(rigs):
    c, eng = rigs("N16")
    picks = [2, 0, 2]
    g = spf_amd.FheCircuit(eng)
    direct = chain_job(g, c, picks)
    g.run()
    n_nodes = g.stats()["nodes"]
    g.close()
    rec = spf_amd.RecordedCircuit(c.P.N)
    ins = [rec.add_input(GLWE, c.x[i]) for i in range(KC.ITEMS)]
    first = [[G.add_node(rec, kind, param, ins[i]) for i in picks] for _, kind, param in G.modes(c)]
    second = [rec.add_glwe_trace(n) for n in first[0]]
    third = [rec.add_glwe_keyswitch(G.SECOND_SLOT, n) for n in second]
    for n in first[0] + first[1] + first[2] + second + third:
        rec.add_output(n, GLWE)
    h, outs = rec.lower(eng)
    h.run()
    assert h.stats()["nodes"] == n_nodes == KC.ITEMS + 5 * len(picks)
    h.close()
    assert G.same_words(np.stack(outs), np.stack(direct))
    for got, want in zip(outs, chain_by_oracle(c, picks)):
        assert G.same_words(got, want)
    again = spf_amd.RecordedCircuit.from_arrays(rec.arrays(), rec.kind, rec.host, c.P.N)
    assert again.op == rec.op and again.param == rec.param and again.inputs == rec.inputs
