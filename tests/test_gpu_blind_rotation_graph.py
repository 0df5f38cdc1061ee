"""Blind rotation by an encrypted shift as gate-graph nodes (`spf_graph_add_blind_rotation`, include/spf_hip.h): one rotate-fused
CMUX node per bit, all nodes of a level with one rotation in ONE launch over a pointer table.  Every comparison is on words
(tests/blind_rotation_graph_cases.py `same_words`): against the oracle's glwe_mul_xn + cmux loop, against the same graph written
with MulXN(2N - r) + CMux nodes, and against `Engine.blind_rotation`.  The argument checks need a graph, hence a context, hence a
device: they are here and not among the CPU tests."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import blind_rotation_graph_cases as K
from tests.util import random_glwe, to_engine_params

pytestmark = pytest.mark.gpu
P = O.DEFAULT_128.replace(lwe_n=1)


@pytest.fixture(scope="module")
def eng():
    e = spf_amd.Engine(to_engine_params(P))
    yield e
    e.close()


@pytest.fixture(scope="module")
def shared():
    """computed once, read by every case: 257 GLWEs and 11 selectors"""
    glwe, sels = random_glwe(0xB60, 257, P.glwe_len), K.random_selectors(0xB61, 11, P)
    glwe.setflags(write=False)
    sels.setflags(write=False)
    return glwe, sels


CASES = [(items, n_bits, log_stride) for items in (1, 256, 257) for n_bits, log_stride in ((1, 0), (1, 10), (3, 8))] + [(1, 11, 0)]


@pytest.mark.parametrize("items,n_bits,log_stride", CASES, ids=[f"items{a}-bits{b}-stride{c}" for a, b, c in CASES])
def test_constructor_graph_against_the_oracle_the_composed_graph_and_the_engine(eng, shared, items, n_bits, log_stride):
    glwe, sels = shared[0][:items].copy(), shared[1][:n_bits].copy()
    g, outs = K.rotation_graph(eng, glwe, sels, log_stride)
    g.run()
    # every level of this graph is one launch of the rotate step: the last one names the shape of all of them
    assert eng.last_cmux_kernel() == (K.FOUR_WAVE_SCATTERED if items <= 256 else K.PER_WG_SCATTERED)
    st = g.stats()
    assert st == {"nodes": n_bits + items * (1 + n_bits), "levels": n_bits, "launches": n_bits}, st
    assert np.array_equal(glwe, shared[0][:items]) and K.same_words(sels, shared[1][:n_bits])      # inputs unchanged
    got = np.stack(outs)

    h, houts = K.rotation_graph(eng, glwe, sels, log_stride, composed=True)
    h.run()
    assert not eng.last_cmux_kernel().endswith("scattered>")
    hst = h.stats()
    assert hst["levels"] == st["levels"] + n_bits and hst["launches"] == st["launches"] + n_bits, (st, hst)
    assert K.same_words(got, np.stack(houts))
    h.close()

    shift = np.ascontiguousarray(np.broadcast_to(sels, (items,) + sels.shape))
    assert K.same_words(got, eng.blind_rotation(shift, glwe, log_stride))
    del shift

    for b in sorted({0, items // 2, items - 2, items - 1} & set(range(items))):
        assert K.same_words(got[b], K.oracle_loop(glwe[b], sels, log_stride)), b

    # run again on new contents of the first input: the nodes read their operands where they lie, every run
    g._keep[n_bits][...] = glwe[0] = random_glwe(0xB62 + items, 1, P.glwe_len)[0]
    g.run()
    assert K.same_words(outs[0], K.oracle_loop(glwe[0], sels, log_stride))
    g.close()


def test_chains_share_launches_by_level_and_rotation(eng, shared):
    """two chains with the same (n_bits, log_stride) share every launch; with different log_stride none; selectors may repeat,
    come from any level and the new nodes are operands like any other"""
    glwe, sels = shared[0][:2].copy(), shared[1][:3].copy()

    def run(strides, repeat=False):
        g = spf_amd.FheCircuit(eng)
        s = [g.add_input(ValueKind.GGSW1, v) for v in sels]
        if repeat:
            s = [s[0], s[1], s[0]]
        outs = [g.add_output(g.add_blind_rotation(g.add_input(ValueKind.GLWE1, x), s, ls), ValueKind.GLWE1)
                for x, ls in zip(glwe, strides)]
        g.run()
        st = g.stats()
        g.close()
        return st, outs

    st, outs = run((2, 2))
    assert st["levels"] == 3 and st["launches"] == 3, st
    st2, outs2 = run((2, 5))
    assert st2["levels"] == 3 and st2["launches"] == 6, st2
    assert K.same_words(outs[0], outs2[0])
    for b, ls in ((0, 2), (1, 5)):
        assert K.same_words(outs2[b], K.oracle_loop(glwe[b], sels, ls)), b
    st3, outs3 = run((0, 0), repeat=True)
    assert st3["launches"] == 3
    assert K.same_words(outs3[1], K.oracle_loop(glwe[1], sels[[0, 1, 0]], 0))

    # a chain on a computed operand, its result an operand of NOT and the source of an unpack
    g = spf_amd.FheCircuit(eng)
    s = [g.add_input(ValueKind.GGSW1, v) for v in sels[:2]]
    x = g.add_op(FheOp.Not, [g.add_input(ValueKind.GLWE1, glwe[0])])
    rot = g.add_blind_rotation(x, s, 4)
    out_not = g.add_output(g.add_op(FheOp.Not, [rot]), ValueKind.GLWE1)
    bits = [g.add_output(b, ValueKind.LWE1) for b in g.add_unpack(rot, 3)]
    g.run()
    assert g.stats() == {"nodes": 2 + 2 + 2 + 1 + 3, "levels": 4, "launches": 5}
    want = K.oracle_loop(O.glwe_not(glwe[0], P.N, P.k), sels[:2], 4)
    assert K.same_words(out_not, O.glwe_not(want, P.N, P.k))
    for i in range(3):
        assert K.same_words(bits[i], O.sample_extract(want, i, P.N, P.k)), i
    g.close()


def test_bad_arguments_are_refused_and_the_graph_stays_usable(eng, shared):
    glwe, sels = shared[0][:1].copy(), shared[1][:2].copy()
    g = spf_amd.FheCircuit(eng)
    s = [g.add_input(ValueKind.GGSW1, v) for v in sels]
    x = g.add_input(ValueKind.GLWE1, glwe[0])
    lib, n_nodes = eng._lib, g.stats()["nodes"]
    arr = (C.c_uint32 * 12)(*([s[0]] * 12))
    node = C.c_uint32(77)

    def refused(status_call, word):
        assert status_call() == 1
        assert word in lib.spf_last_error(eng._h).decode(), lib.spf_last_error(eng._h)
        assert g.stats()["nodes"] == n_nodes and node.value == 77      # nothing recorded

    add = lib.spf_graph_add_blind_rotation
    refused(lambda: add(g._g, x, arr, 0, 0, C.byref(node)), "n_bits")
    refused(lambda: add(g._g, x, arr, 12, 0, C.byref(node)), "n_bits + log_stride")
    refused(lambda: add(g._g, x, arr, 2, 10, C.byref(node)), "n_bits + log_stride")             # 2 + 10 = log2 N + 1
    refused(lambda: add(g._g, x, (C.c_uint32 * 2)(s[0], x), 2, 0, C.byref(node)), "selector is not an L1 GGSW")
    refused(lambda: add(g._g, s[0], arr, 2, 0, C.byref(node)), "operand is not an L1 GLWE")
    refused(lambda: add(g._g, n_nodes, arr, 2, 0, C.byref(node)), "not a node")
    refused(lambda: add(g._g, x, (C.c_uint32 * 2)(s[0], n_nodes), 2, 0, C.byref(node)), "not a node")
    refused(lambda: add(g._g, x, None, 2, 0, C.byref(node)), "null")
    refused(lambda: add(g._g, x, arr, 2, 0, None), "null")
    assert add(None, x, arr, 2, 0, C.byref(node)) == 1
    with pytest.raises(spf_amd.SpfError, match="n_bits"):
        g.add_blind_rotation(x, [])
    with pytest.raises(spf_amd.SpfError, match="log_stride"):
        g.add_blind_rotation(x, s, 10)
    with pytest.raises(spf_amd.SpfError, match="log_stride"):
        g.add_blind_rotation(x, s, -1)
    out = g.add_output(g.add_blind_rotation(x, s, 9), ValueKind.GLWE1)                           # 2 + 9 = log2 N: accepted
    g.run()
    assert K.same_words(out, K.oracle_loop(glwe[0], sels, 9))
    g.close()


def test_recorded_circuit_lowers_to_the_same_words(eng, shared):
    glwe, sels = shared[0][:2].copy(), shared[1][:3].copy()
    rec = spf_amd.RecordedCircuit(P.N)
    rec, _ = K.rotation_graph(eng, glwe, sels, 1, circuit=rec)
    assert rec.outputs == [6, 10] and rec.op[4:7] == [spf_amd.graph.NODE_ROT_CMUX] * 3 and rec.param[4:7] == [2, 4, 8]
    g, outs = rec.lower(eng)
    g.run()
    assert g.stats() == {"nodes": len(rec.op), "levels": 3, "launches": 3}
    for b in range(2):
        assert K.same_words(outs[b], K.oracle_loop(glwe[b], sels, 1)), b
    g.close()
    a = rec.arrays()
    again = spf_amd.RecordedCircuit.from_arrays(a, rec.kind, rec.host, P.N)
    assert again.op == rec.op and again.param == rec.param and again.inputs == rec.inputs and again.outputs == rec.outputs


def test_group_jobs_carry_the_nodes_through_a_merge(eng, shared):
    """three jobs of 3 items over a group [0, 0]: one member runs two of them merged into one graph; the words of one context"""
    sels = shared[1][:2].copy()
    glwes = [shared[0][3 * j:3 * j + 3].copy() for j in range(3)]
    grp = spf_amd.Group(to_engine_params(P), devices=[0, 0])
    jobs = []
    try:
        for j in range(3):
            jobs.append(K.rotation_graph(grp, glwes[j], sels, 3 + j))
        grp.run_graphs([g for g, _ in jobs])
        assert sorted(g.member() for g, _ in jobs) in ([0, 0, 1], [0, 1, 1])
        for j, (g, outs) in enumerate(jobs):
            one, want = K.rotation_graph(eng, glwes[j], sels, 3 + j)
            one.run()
            assert K.same_words(np.stack(outs), np.stack(want)), j
            one.close()
    finally:
        for g, _ in jobs:
            g.close()
        grp.close()


@pytest.mark.parametrize("Q", [K.SMALL16, K.TEST1], ids=["N16k1", "N128k2"])
def test_shift_right_by_an_encrypted_amount_on_generic_contexts(Q):
    """x >> s, a packed 8-bit x and a packed 3-bit s, every s in one graph: unpack(s), KeyswitchL1toL0 and CircuitBootstrap per
    bit, the rotation, unpack(8).  Word-equal to the oracle running the same steps, and — the oracle's own result decodes for all
    eight shifts under these keys (checked without a device: the decode below is of the ORACLE's words, which the graph's equal)
    — every s gives the bits of x >> s.  The wrapped coefficients land, negated, at N - s .. N - 1, above bit 8."""
    ks = O.gen_keyset(0x5EED0009, Q)
    r = O.Rng(0x7A12)
    ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, Q), O.gen_ssk_fft(r, ks.glwe_sk, Q)
    e = spf_amd.Engine(K.engine_params(Q))
    e.load_bootstrap_key(ks.bsk_fft)
    e.load_keyswitch_key(ks.ksk)
    e.load_automorphism_key(ak)
    e.load_scheme_switch_key(ssk)
    rng, x = O.Rng(0xB0B), 0xB5
    cts = [(K.packed_glwe(rng, ks.glwe_sk, Q, x, 8), K.packed_glwe(rng, ks.glwe_sk, Q, s, 3)) for s in range(8)]
    g = spf_amd.FheCircuit(e)
    s_nodes = [g.add_input(ValueKind.GLWE1, s_ct) for _, s_ct in cts]     # (side by side: their unpack needs no gather)
    x_nodes = [g.add_input(ValueKind.GLWE1, x_ct) for x_ct, _ in cts]
    outs = [K.shift_right_graph(g, xn, sn, 3, 8) for xn, sn in zip(x_nodes, s_nodes)]
    g.run()
    assert e.last_cmux_kernel() == K.GENERIC_ROT
    st = g.stats()
    # unpack(s), keyswitch, bootstrap, three rotation levels of eight nodes each in one launch, unpack(x)
    assert st["levels"] == 7 and st["launches"] == 7, st
    for s, ((x_ct, s_ct), (rot, lwes)) in enumerate(zip(cts, outs)):
        want_rot, want_lwes = K.oracle_shift_right(Q, ks, ak, ssk, x_ct, s_ct, 3, 8)
        assert K.same_words(rot, want_rot), s
        for j in range(8):
            assert K.same_words(lwes[j], want_lwes[j]), (s, j)
        bits = [O.decode(O.decrypt_lwe_raw(want_lwes[j], ks.glwe_sk), 1) for j in range(8)]
        assert sum(b << j for j, b in enumerate(bits)) == x >> s, (s, bits)
    g.close()
    e.close()
