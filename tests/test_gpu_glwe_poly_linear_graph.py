"""The plaintext polynomial linear maps over GLWE ciphertexts as gate-graph nodes (`spf_graph_add_glwe_poly_linear`,
include/spf_hip.h), on the tuned DEFAULT_128 kernels ((N, k) = (2048, 1)) and on generic contexts at (128, 2) — W = 384 words is no
multiple of 256, three polynomials — and (16, 1), where N is below the workgroup.  Every node is an output, so every word of the
arena's results is compared (tests/glwe_poly_graph_cases.py): against `poly_linear_ref` on the operand nodes' own words, against
`Engine.glwe_poly_linear` on the same rows, and against the oracle for the nodes around a layer.  One case decrypts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import glwe_poly_cases as GC
from tests import glwe_poly_graph_cases as G
from tests.blind_rotation_graph_cases import oracle_loop, random_selectors
from tests.util import random_glwe, random_lwe_batch

pytestmark = pytest.mark.gpu
GLWE = ValueKind.GLWE1


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


def run_stats(g):
    g.run()
    return g.stats()


# ---- 1. scattered operands, both rows kernels ----------------------------------------------------------------------------------

@pytest.mark.parametrize("M,K", G.SCATTERED_SHAPES)
@pytest.mark.parametrize("which", G.CONTEXTS)
def test_scattered_operands_take_one_launch_of_a_rows_kernel(rigs, monkeypatch, which, M, K):
    P, eng, ks = rigs(which)
    k1, N = G.dims(P)
    base, _, _, _ = G.pool_graph(eng, P, 3, G.LAYERS, K, M, 0xA10 + K, with_layers=False)
    base_stats = run_stats(base)
    base.close()
    variants = G.slots(M, K, N)
    g, pool, pk, outs = G.pool_graph(eng, P, 3, G.LAYERS, K, M, 0xA10 + K)
    rows = None
    for path in (None, "lds"):
        G.set_path(monkeypatch, path)
        for name, (triple, bias) in variants.items():
            G.load(eng, 3, triple, M, K, bias)                       # the slot is read when the graph runs: one graph, every slot
            assert eng.glwe_poly_slot_shape(3)[:2] == (M, K) and eng.glwe_poly_slot_shape(3)[3] == (bias is not None)
            st = run_stats(g)
            assert eng.last_glwe_poly_kernel() == G.rows_kernel_name(triple, path), (name, path)
            # the layers of the level are ONE launch on top of the pool's, whatever layers, M and K
            assert st == {"nodes": base_stats["nodes"] + G.LAYERS * M, "levels": max(base_stats["levels"], 3 if K > 1 else 1),
                          "launches": base_stats["launches"] + 1}, (st, base_stats)
            if rows is None:
                rows = G.operand_rows(pool, pk, P)
                assert G.same_words(np.stack(pool.outs), pool.by_oracle())      # the nodes around, by the oracle
            got = G.stack(outs, P)
            assert rows.shape == (G.LAYERS, K, k1, N) and got.shape == (G.LAYERS, M, k1, N)
            want = GC.poly_linear_ref(rows, triple, M, K, bias)
            bad = np.argwhere((got != want).any(axis=-1))
            assert bad.size == 0, (which, M, K, name, path, bad[:8])
            if path is None:
                assert G.same_words(got, eng.glwe_poly_linear(3, rows)), (name, path)
    g.close()


# ---- 2. in-place operands ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", [None, "lds"])
@pytest.mark.parametrize("which", G.CONTEXTS)
def test_in_place_operands_go_to_the_batch_kernels(rigs, monkeypatch, which, path):
    P, eng, ks = rigs(which)
    k1, N = G.dims(P)
    G.set_path(monkeypatch, path)
    layers, K, M1, M2 = 2, 3, G.VT + 1, 2
    general = GC.csr(GC.random_polys(0xA20, M1, K, N, terms=3, cls="seams", empty_every=4), M1, K)
    constants = GC.csr(GC.random_polys(0xA21, M2, M1, N, terms=2, cls="constants"), M2, M1)
    bias = GC.random_bias(0xA22, M1, N)
    G.load(eng, 6, general, M1, K, bias)
    G.load(eng, 7, constants, M2, M1)
    x = random_glwe(0xA23, 2 * layers * K, P.glwe_len)

    def words_of(outs):
        return np.stack(outs).reshape(len(outs), k1, N)

    # set A: the K operands of every layer are the consecutive results of ONE XOR group, in its order
    def xor_graph(with_layers):
        g = spf_amd.FheCircuit(eng)
        ins = [g.add_input(GLWE, v) for v in x]
        xs = [g.add_op(FheOp.GlweAdd, [ins[2 * j], ins[2 * j + 1]]) for j in range(layers * K)]
        row_outs = [g.add_output(n, GLWE) for n in xs]
        a = [g.add_glwe_poly_linear(6, xs[q * K:(q + 1) * K]) for q in range(layers)] if with_layers else []
        return g, row_outs, [[g.add_output(n, GLWE) for n in layer] for layer in a]

    g, _, _ = xor_graph(False)
    base = run_stats(g)
    g.close()
    g, row_outs, a_outs = xor_graph(True)
    st = run_stats(g)
    assert eng.last_glwe_poly_kernel() == GC.kernel_name(general, path) == GC.LDS
    assert st == {"nodes": base["nodes"] + layers * M1, "levels": 2, "launches": base["launches"] + 1}, (st, base)   # both layers: ONE launch
    g.close()
    rows = words_of(row_outs).reshape(layers, K, k1, N)
    assert G.same_words(rows.reshape(layers * K, -1), np.stack([O.glwe_xor(x[2 * j], x[2 * j + 1], P.N, P.k) for j in range(layers * K)]))
    assert G.same_words(G.stack(a_outs, P), GC.poly_linear_ref(rows, general, M1, K, bias))
    assert G.same_words(G.stack(a_outs, P), eng.glwe_poly_linear(6, rows))
    # set B: the consecutive results of ONE pack group
    g = spf_amd.FheCircuit(eng)
    ins = [g.add_input(GLWE, v) for v in x[:2 * K]]
    packs = [g.add_pack([ins[2 * j + 1], ins[2 * j]]) for j in range(K)]
    row_outs = [g.add_output(n, GLWE) for n in packs]
    outs = [g.add_output(n, GLWE) for n in g.add_glwe_poly_linear(6, packs)]
    st = run_stats(g)
    assert eng.last_glwe_poly_kernel() == GC.LDS and st == {"nodes": 3 * K + M1, "levels": 2, "launches": 2}, st    # pack rows | the layer
    g.close()
    rows = words_of(row_outs).reshape(1, K, k1, N)
    assert G.same_words(words_of(outs)[None], GC.poly_linear_ref(rows, general, M1, K, bias))
    assert G.same_words(words_of(outs)[None], eng.glwe_poly_linear(6, rows))
    # set C: the M1 results of a previous polynomial layer (itself over scattered inputs), on a constants-only slot
    g = spf_amd.FheCircuit(eng)
    ins = [g.add_input(GLWE, v) for v in x[:K]]
    first = g.add_glwe_poly_linear(6, ins[::-1])
    second = g.add_glwe_poly_linear(7, first)
    outs = [[g.add_output(n, GLWE) for n in layer] for layer in (first, second)]
    st = run_stats(g)
    assert eng.last_glwe_poly_kernel() == GC.kernel_name(constants, path)
    assert st == {"nodes": K + M1 + M2, "levels": 2, "launches": 2}, st
    g.close()
    mid = GC.poly_linear_ref(x[:K][::-1].reshape(1, K, k1, N), general, M1, K, bias)
    assert G.same_words(words_of(outs[0])[None], mid)
    assert G.same_words(words_of(outs[1])[None], GC.poly_linear_ref(mid, constants, M2, M1))
    assert G.same_words(words_of(outs[1])[None], eng.glwe_poly_linear(7, words_of(outs[0])[None]))


# ---- 3. consumers --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", G.CONTEXTS)
def test_every_kind_of_consumer_reads_a_layers_rows(rigs, monkeypatch, which):
    """the rows of one layer as the source of an unpack and of a SampleExtract, the low and the high operand of a CMUX, the
    accumulator of a blind rotation, the TABLE of a univariate bootstrap and the operands of another layer: each against the
    oracle walking the layer's own output words"""
    P, eng, ks = rigs(which)
    k1, N = G.dims(P)
    G.set_path(monkeypatch, None)
    M, K, M2 = 4, 2, 2
    w = GC.csr(GC.random_polys(0xA30, M, K, N, terms=2, cls="seams"), M, K)
    w2 = GC.csr(GC.random_polys(0xA31, M2, 3, N, terms=2, cls="mixed"), M2, 3)
    bias = GC.random_bias(0xA32, M, N)
    G.load(eng, 8, w, M, K, bias)
    G.load(eng, 9, w2, M2, 3)
    x = random_glwe(0xA33, 3, P.glwe_len)
    sels = random_selectors(0xA34, 2, P)
    l0 = random_lwe_batch(0xA35, 1, P.lwe_n)[0]
    g = spf_amd.FheCircuit(eng)
    ins = [g.add_input(GLWE, v) for v in x]
    s = [g.add_input(ValueKind.GGSW1, v) for v in sels]
    lwe = g.add_input(ValueKind.LWE0, l0)
    L = g.add_glwe_poly_linear(8, [ins[1], ins[0]])
    rows_out = [g.add_output(n, GLWE) for n in L]
    bits = [g.add_output(n, ValueKind.LWE1) for n in g.add_unpack(L[0], 3)]
    ext = g.add_output(g.add_op(FheOp.SampleExtract, [L[1]], N - 1), ValueKind.LWE1)
    cm_low = g.add_output(g.add_op(FheOp.CMux, [s[0], L[0], ins[2]]), GLWE)
    cm_high = g.add_output(g.add_op(FheOp.CMux, [s[1], ins[2], L[1]]), GLWE)
    cm_both = g.add_output(g.add_op(FheOp.CMux, [s[0], L[3], L[2]]), GLWE)
    rot = g.add_output(g.add_blind_rotation(L[2], s, 1), GLWE)
    pbs = g.add_output(g.add_op(FheOp.PBS_UNIVARIATE, [lwe, L[3]]), ValueKind.LWE1)
    again = [g.add_output(n, GLWE) for n in g.add_glwe_poly_linear(9, [L[1], L[3], L[1]])]
    g.run()
    assert eng.last_glwe_poly_kernel() == G.LDS_ROWS                 # (the second layer's operands: rows 1, 3, 1)
    g.close()
    rows = np.stack(rows_out)
    assert G.same_words(rows.reshape(1, M, k1, N), GC.poly_linear_ref(x[[1, 0]].reshape(1, K, k1, N), w, M, K, bias))
    cbs = (P.N, P.k, P.cbs_radix_log, P.cbs_count)
    for j in range(3):
        assert G.same_words(bits[j], O.sample_extract(rows[0], j, P.N, P.k)), j
    assert G.same_words(ext, O.sample_extract(rows[1], N - 1, P.N, P.k))
    assert G.same_words(cm_low, O.cmux(rows[0], x[2], sels[0], *cbs))
    assert G.same_words(cm_high, O.cmux(x[2], rows[1], sels[1], *cbs))
    assert G.same_words(cm_both, O.cmux(rows[3], rows[2], sels[0], *cbs))
    assert G.same_words(rot, oracle_loop(rows[2], sels, 1, P))
    assert G.same_words(pbs, O.pbs_univariate(l0, rows[3], ks.bsk_fft, P))
    assert G.same_words(np.stack(again).reshape(1, M2, k1, N), GC.poly_linear_ref(rows[[1, 3, 1]].reshape(1, 3, k1, N), w2, M2, 3))


# ---- 4. the decrypt-level case -------------------------------------------------------------------------------------------------

def test_a_shifted_packed_integer_added_to_another_decrypts_to_the_model(rigs, monkeypatch):
    """two packed 8-bit integers, the slot w = [X^s, 1], the layer and add_unpack of 8 + s bits in ONE graph: the bits of
    (a << s) ^ b (tests/test_glwe_poly_graph_host.py holds the oracle's own walk to the same model)"""
    P, eng, ks = rigs("tuned")
    k1, N = G.dims(P)
    G.set_path(monkeypatch, None)
    for i, (a, b, s) in enumerate(G.MODEL_CASES):
        G.load(eng, 20 + i, G.model_slot(s), 1, 2)
        x = G.model_encrypt(P, ks, a, b)
        g = spf_amd.FheCircuit(eng)
        ins = [g.add_input(GLWE, v) for v in x]
        layer = g.add_glwe_poly_linear(20 + i, ins)
        packed = g.add_output(layer[0], GLWE)
        bits = [g.add_output(n, ValueKind.LWE1) for n in g.add_unpack(layer[0], G.BITS + s)]
        st = run_stats(g)
        assert st == {"nodes": 3 + G.BITS + s, "levels": 2, "launches": 2}, st           # the layer (in place: two inputs) | the unpack
        g.close()
        assert G.same_words(packed.reshape(1, 1, k1, N), GC.poly_linear_ref(x.reshape(1, 2, k1, N), G.model_slot(s), 1, 2))
        for j in range(G.BITS + s):
            assert G.same_words(bits[j], O.sample_extract(packed, j, P.N, P.k)), (i, j)
        assert G.model_decrypt(ks, bits) == G.model(a, b, s), (a, b, s)


# ---- 5. the slots at run time --------------------------------------------------------------------------------------------------

def test_errors_of_the_run_and_the_graph_still_runs_once_the_weights_are_there(monkeypatch):
    P = G.keys_of("n16k1")[0]
    k1, N = G.dims(P)
    G.set_path(monkeypatch, None)
    eng = spf_amd.Engine(G.engine_params(P))
    try:
        x = random_glwe(0xA80, 5, P.glwe_len)
        g = spf_amd.FheCircuit(eng)
        ins = [g.add_input(GLWE, v) for v in x]
        outs = [g.add_output(n, GLWE) for n in g.add_glwe_poly_linear(40, ins[::-1], 3)]   # built before the slot is loaded
        with pytest.raises(spf_amd.SpfError) as e:
            g.run()
        assert e.value.status == G.NO_KEY and "slot 40" in str(e.value), str(e.value)
        G.load(eng, 40, GC.csr(GC.random_polys(0xA81, 7, 6, N, terms=1), 7, 6), 7, 6)
        with pytest.raises(spf_amd.SpfError) as e:
            g.run()
        assert e.value.status == G.INVALID and "7 x 6" in str(e.value) and "3 x 5" in str(e.value), str(e.value)
        w, b = GC.csr(GC.random_polys(0xA82, 3, 5, N, terms=2), 3, 5), GC.random_bias(0xA83, 3, N)
        G.load(eng, 40, w, 3, 5, b)
        g.run()
        assert eng.last_glwe_poly_kernel() == G.LDS_ROWS
        assert G.same_words(np.stack(outs).reshape(1, 3, k1, N), GC.poly_linear_ref(x[::-1].reshape(1, 5, k1, N), w, 3, 5, b))
        g.close()
    finally:
        eng.close()


def test_a_slot_loaded_again_between_runs_gives_the_new_weights(rigs, monkeypatch):
    P, eng, ks = rigs("n128k2")
    G.set_path(monkeypatch, None)
    G.reload_rounds(eng, P)


def test_a_reload_after_the_capture_drops_the_replayed_graph():
    """SPF_GRAPH_CAPTURE=1 is read once per process, hence the child: the second run captures, the third replays, the slots are
    loaded again (their old images are freed), the fourth run must give the new weights' words"""
    code = ("import spf_amd\n"
            "from tests import glwe_poly_graph_cases as G\n"
            "P = G.keys_of('n128k2')[0]\n"
            "eng = spf_amd.Engine(G.engine_params(P))\n"
            "G.reload_rounds(eng, P)\n"
            "eng.close()\nprint('reload ok')\n")
    env = dict(os.environ, SPF_GRAPH_CAPTURE="1")
    env.pop("SPF_GLWE_POLY_PATH", None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, env=env, timeout=300)
    assert r.returncode == 0 and "reload ok" in r.stdout, r.stderr[-3000:]


# ---- 6. grouping ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", G.CONTEXTS)
def test_layers_of_one_slot_and_level_are_one_launch(rigs, monkeypatch, which):
    P, eng, ks = rigs(which)
    k1, N = G.dims(P)
    G.set_path(monkeypatch, None)
    M, K = 3, 2
    w0, b0 = GC.csr(GC.random_polys(0xA40, M, K, N, terms=2, cls="seams"), M, K), GC.random_bias(0xA41, M, N)
    w1 = GC.csr(GC.random_polys(0xA42, M, K, N, terms=2, cls="constants"), M, K)
    G.load(eng, 10, w0, M, K, b0)
    G.load(eng, 11, w1, M, K)
    x = random_glwe(0xA43, 2 * K, P.glwe_len).reshape(2, K, k1, N)

    def graph(plan):
        """plan: [(slot, which pair of inputs)] -> (stats, [(M, k+1, N) words per entry])"""
        g = spf_amd.FheCircuit(eng)
        ins = [[g.add_input(GLWE, v) for v in pair] for pair in x]
        outs = [[g.add_output(n, GLWE) for n in g.add_glwe_poly_linear(slot, ins[q][::-1])] for slot, q in plan]
        st = run_stats(g)
        g.close()
        return st, [np.stack(o).reshape(M, k1, N) for o in outs]

    def want(w, q, b=None):
        return GC.poly_linear_ref(x[q][::-1][None], w, M, K, b)[0]

    base, _ = graph([])
    st, got = graph([(10, 0), (10, 1)])                               # the same (slot, M, K) on one level: one group
    assert st == {"nodes": 2 * K + 2 * M, "levels": 1, "launches": base["launches"] + 1}, (st, base)
    assert G.same_words(got[0], want(w0, 0, b0)) and G.same_words(got[1], want(w0, 1, b0)) and not np.array_equal(got[0], got[1])
    st, got = graph([(10, 0), (11, 1)])                               # two slots on one level: two
    assert st["launches"] == base["launches"] + 2 and st["levels"] == 1, st
    assert G.same_words(got[0], want(w0, 0, b0)) and G.same_words(got[1], want(w1, 1))


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_the_graph_stays_usable(rigs, monkeypatch):
    P, eng, ks = rigs("tuned")
    k1, N = G.dims(P)
    G.set_path(monkeypatch, None)
    w, b = GC.csr(GC.random_polys(0xA70, 2, 2, N, terms=2), 2, 2), GC.random_bias(0xA71, 2, N)
    G.load(eng, 30, w, 2, 2, b)
    x = random_glwe(0xA72, 2, P.glwe_len)
    g = spf_amd.FheCircuit(eng)
    a, a2 = (g.add_input(GLWE, v) for v in x)
    l1 = g.add_input(ValueKind.LWE1, random_lwe_batch(0xA73, 1, P.k * P.N)[0])
    glev = g.add_trivial(ValueKind.GLEV1, 1)
    lib, n_nodes = eng._lib, g.stats()["nodes"]
    out = (C.c_uint32 * (G.MAX_ROWS + 1))(*([77] * (G.MAX_ROWS + 1)))
    add = lib.spf_graph_add_glwe_poly_linear

    def refused(status_call, word):
        assert status_call() == 1
        message = lib.spf_last_error(eng._h).decode()
        assert message.startswith("graph polynomial linear map: ") and word in message, message
        assert g.stats()["nodes"] == n_nodes and set(out) == {77}       # nothing recorded

    two = (C.c_uint32 * 2)(a, a2)
    refused(lambda: add(g._g, G.SLOTS, two, 2, 2, out), "slot 64 >= SPF_GLWE_POLY_SLOTS = 64")
    refused(lambda: add(g._g, 30, two, 0, 2, out), "K must be in 1 ..= 2^32 - 1")
    refused(lambda: add(g._g, 30, two, 1 << 32, 2, out), "K must be in 1 ..= 2^32 - 1")
    refused(lambda: add(g._g, 30, two, 2, 0, out), "M must be in 1 ..= SPF_GLWE_POLY_MAX_ROWS = 4096")
    refused(lambda: add(g._g, 30, two, 2, G.MAX_ROWS + 1, out), "M must be in 1 ..= SPF_GLWE_POLY_MAX_ROWS = 4096")
    refused(lambda: add(g._g, 30, None, 2, 2, out), "null pointer")
    refused(lambda: add(g._g, 30, two, 2, 2, None), "null pointer")
    refused(lambda: add(g._g, 30, (C.c_uint32 * 2)(a, n_nodes), 2, 2, out), "operand is not a node of this graph")
    refused(lambda: add(g._g, 30, (C.c_uint32 * 2)(a, l1), 2, 2, out), "operand is not an L1 GLWE")
    refused(lambda: add(g._g, 30, (C.c_uint32 * 2)(glev, a), 2, 2, out), "operand is not an L1 GLWE")
    assert add(None, 30, two, 2, 2, out) == 1
    with pytest.raises(spf_amd.SpfError, match="K = 0"):
        g.add_glwe_poly_linear(30, [])
    with pytest.raises(spf_amd.SpfError) as e:
        g.add_glwe_poly_linear(31, [a, a2])                              # M=None asks the engine: the slot is empty
    assert e.value.status == G.NO_KEY and g.stats()["nodes"] == n_nodes
    rows = g.add_glwe_poly_linear(30, [a2, a])                           # ... and the graph still runs
    assert rows == [n_nodes, n_nodes + 1]
    outs = [g.add_output(n, GLWE) for n in rows]
    g.run()
    assert G.same_words(np.stack(outs).reshape(1, 2, k1, N), GC.poly_linear_ref(x[::-1].reshape(1, 2, k1, N), w, 2, 2, b))
    g.close()
    g = spf_amd.FheCircuit(eng)                                          # M at the limit: accepted (not run: 4096 GLWEs of 32 KiB)
    one = g.add_input(GLWE, x[0])
    assert g.add_glwe_poly_linear(30, [one] * 3, G.MAX_ROWS) == list(range(1, 1 + G.MAX_ROWS))
    g.close()


# ---- 8. group, 9. recorded circuit ---------------------------------------------------------------------------------------------

def two_layer_job(g, x, slot_a, slot_b, M1=None, M2=None):
    xs = [g.add_input(GLWE, row) for row in x]
    a = g.add_glwe_poly_linear(slot_a, xs[::-1], M1)
    b = g.add_glwe_poly_linear(slot_b, a, M2)
    return [g.add_output(n, GLWE) for n in a + b]


def test_group_jobs_carry_the_nodes_through_a_merge(rigs, monkeypatch):
    """two jobs with the same layers over members [0, 0] — whichever way they are dealt, the words are those of the graphs run
    alone on one context"""
    P, eng, ks = rigs("n128k2")
    k1, N = G.dims(P)
    G.set_path(monkeypatch, None)
    K, M1, M2 = 3, G.VT + 1, 2
    wa, ba = GC.csr(GC.random_polys(0xA90, M1, K, N, terms=2, cls="seams"), M1, K), GC.random_bias(0xA91, M1, N)
    wb = GC.csr(GC.random_polys(0xA92, M2, M1, N, terms=2, cls="constants"), M2, M1)
    xs = random_glwe(0xA93, 2 * K, P.glwe_len).reshape(2, K, -1)
    G.load(eng, 50, wa, M1, K, ba)
    G.load(eng, 51, wb, M2, M1)
    alone = []
    for x in xs:
        g = spf_amd.FheCircuit(eng)
        outs = two_layer_job(g, x, 50, 51)
        g.run()
        g.close()
        alone.append(np.stack(outs))
        mid = GC.poly_linear_ref(x[::-1].reshape(1, K, k1, N), wa, M1, K, ba)
        assert G.same_words(alone[-1].reshape(M1 + M2, k1, N), np.concatenate([mid[0], GC.poly_linear_ref(mid, wb, M2, M1)[0]]))
    grp = spf_amd.Group(G.engine_params(P), devices=[0, 0])
    jobs = []
    try:
        g = spf_amd.FheCircuit(grp)
        jobs.append((g, two_layer_job(g, xs[0], 50, 51, M1, M2)))       # built before the group's slots are loaded
        with pytest.raises(spf_amd.SpfError) as e:
            grp.run_graphs([g])                                          # the merged graph checks the member's slots
        assert e.value.status == G.NO_KEY
        grp.load_glwe_poly_weights(50, wa, ba, shape=(M1, K))
        grp.load_glwe_poly_weights(51, wb, shape=(M2, M1))
        g = spf_amd.FheCircuit(grp)
        jobs.append((g, two_layer_job(g, xs[1], 50, 51)))               # (M=None: the group is asked for the slots' shapes)
        grp.run_graphs([g for g, _ in jobs])
        for j, (_, outs) in enumerate(jobs):
            assert G.same_words(np.stack(outs), alone[j]), j
    finally:
        for g, _ in jobs:
            g.close()
        grp.close()


def test_recorded_circuit_lowers_to_the_same_words(rigs, monkeypatch):
    P, eng, ks = rigs("n16k1")
    G.set_path(monkeypatch, None)
    K, M1, M2 = 3, 2, G.VT + 1
    N = P.N
    G.load(eng, 60, GC.csr(GC.random_polys(0xAA0, M1, K, N, terms=2, cls="seams"), M1, K), M1, K, GC.random_bias(0xAA1, M1, N))
    G.load(eng, 61, GC.csr(GC.random_polys(0xAA2, M2, M1, N, terms=2, cls="mixed"), M2, M1), M2, M1)
    x = random_glwe(0xAA3, K, P.glwe_len)
    g = spf_amd.FheCircuit(eng)
    direct = two_layer_job(g, x, 60, 61)
    g.run()
    g.close()
    rec = spf_amd.RecordedCircuit(P.N)
    two_layer_job(rec, x, 60, 61, M1, M2)
    h, outs = rec.lower(eng)
    h.run()
    assert h.stats()["nodes"] == K + M1 + M2
    h.close()
    assert G.same_words(np.stack(outs), np.stack(direct))
    again = spf_amd.RecordedCircuit.from_arrays(rec.arrays(), rec.kind, rec.host, P.N)
    assert again.op == rec.op and again.param == rec.param and again.inputs == rec.inputs and again._linear == rec._linear
