"""Packed integers in and out of gate graphs: `spf_graph_add_unpack` / `spf_graph_add_pack` (include/spf_hip.h), the node
constructors that stand for `PackedGenericInt::graph_input(ctx).unpack(ctx)` and `.pack(ctx, enc).collect_output(ctx, enc)`
(fluent/packed_dynamic_generic_int_graph_node.rs:24-60, fluent/dynamic_generic_int_graph_nodes.rs:139-200).

Unpack nodes are held word for word to `O.sample_extract(ct, i)` and to a graph of `SampleExtract(i)` nodes; pack nodes to
the reference's MulXN + GlweAdd tree (tests/test_packed_plaintext.py `oracle_tree_pack`) and to `spf_glwe_pack_batch` of the
same rows.  At DEFAULT_128 a packed integer goes through unpack -> KeyswitchL1toL0 -> CircuitBootstrap -> MultiplyGgswGlwe ->
pack and decrypts to itself, and the 32-bit ripple-carry adder of tests/test_gpu_graph.py takes two packed integers and
returns one packed 33-bit sum at the cost of one more level and at most two more launches."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests.test_packed_plaintext import oracle_tree_pack
from tests.util import keyset, random_glwe, to_engine_params

pytestmark = pytest.mark.gpu

# the two generic shapes: the smallest one, and one with k > 1
N16K1 = O.DEFAULT_128.replace(lwe_n=5, lwe_std=0.0, N=16, k=1, glwe_std=0.0, pbs_radix_log=6, pbs_count=2, cbs_radix_log=5,
                              cbs_count=3, ks_radix_log=2, ks_count=6, tr_radix_log=6, tr_count=5, ss_radix_log=5, ss_count=6)
N32K2 = O.DEFAULT_128.replace(lwe_n=5, lwe_std=1e-16, N=32, k=2, glwe_std=1e-16, pbs_radix_log=4, pbs_count=3,
                              cbs_radix_log=4, cbs_count=3, ks_radix_log=4, ks_count=3)
GENERIC = {"N16k1": N16K1, "N32k2": N32K2}
CASES = [(name, which) for name in GENERIC for which in ("1", "2", "N-1", "N")]


def _n_bits(P, which):
    return {"1": 1, "2": 2, "N-1": P.N - 1, "N": P.N}[which]


def _eng_params(P):
    return to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count,
                                       ss_radix_log=P.ss_radix_log, ss_radix_count=P.ss_count)


@pytest.fixture(scope="module")
def generic():
    """keyless generic contexts (unpack, pack and the linear operations need no key)"""
    out = {name: (P, spf_amd.Engine(_eng_params(P))) for name, P in GENERIC.items()}
    yield out
    for _, e in out.values():
        e.close()


def _load_all(e, ks, ak, ssk):
    e.load_bootstrap_key(ks.bsk_fft)
    e.load_keyswitch_key(ks.ksk)
    e.load_automorphism_key(ak)
    e.load_scheme_switch_key(ssk)


@pytest.fixture(scope="module")
def full():
    """DEFAULT_128 under the suite's keys, all four loaded"""
    ks = keyset(0x5EED0001, 637)
    r = O.Rng(0x9AC4)
    ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, ks.params), O.gen_ssk_fft(r, ks.glwe_sk, ks.params)
    eng = spf_amd.Engine(to_engine_params(ks.params))
    _load_all(eng, ks, ak, ssk)
    yield ks, eng
    eng.close()


def _not(x, P):
    y = x.copy()
    y[P.k * P.N] ^= np.uint64(1 << 63)                          # + 2^63 mod 2^64
    return y


def _trivial(bit, P):
    y = np.zeros(P.glwe_len, dtype=np.uint64)
    y[P.k * P.N] = np.uint64(bit << 63)
    return y


@pytest.mark.parametrize("name,which", CASES, ids=[f"{a}-n{b}" for a, b in CASES])
def test_unpack_nodes_equal_sample_extract(generic, name, which):
    P, eng = generic[name]
    n = _n_bits(P, which)
    cts = random_glwe(0x9B00 + n, 2, P.glwe_len)
    g = spf_amd.FheCircuit(eng)
    ins = [g.add_input(ValueKind.GLWE1, x) for x in cts]
    flipped = g.add_op(FheOp.Not, [ins[1]])
    sources = ins + [flipped]                                   # two inputs in one launch, and a computed node one level on
    nodes = [g.add_unpack(s, n) for s in sources]
    assert all(len(b) == n for b in nodes) and len({x for b in nodes for x in b}) == 3 * n
    outs = [[g.add_output(x, ValueKind.LWE1) for x in b] for b in nodes]
    g.run()
    st = g.stats()
    # level 1: ONE unpack launch for both inputs (consecutive in the arena: no gather) + the NOT; level 2: one unpack
    assert st == {"nodes": 3 + 3 * n, "levels": 2, "launches": 3}, st

    h = spf_amd.FheCircuit(eng)                                 # the same from SampleExtract(i) nodes
    hin = [h.add_input(ValueKind.GLWE1, x) for x in cts]
    hsrc = hin + [h.add_op(FheOp.Not, [hin[1]])]
    houts = [[h.add_output(h.add_op(FheOp.SampleExtract, [s], i), ValueKind.LWE1) for i in range(n)] for s in hsrc]
    h.run()
    values = [cts[0], cts[1], _not(cts[1], P)]
    for s in range(3):
        for i in range(n):
            assert np.array_equal(outs[s][i], O.sample_extract(values[s], i, P.N, P.k)), (s, i)
            assert np.array_equal(outs[s][i], houts[s][i]), (s, i)
    # run again on new contents of the first input
    g._keep[0][...] = cts[0] = random_glwe(0x9B80 + n, 1, P.glwe_len)[0]
    g.run()
    assert np.array_equal(outs[0][n - 1], O.sample_extract(cts[0], n - 1, P.N, P.k))
    g.close()
    h.close()


@pytest.mark.parametrize("name,which", CASES, ids=[f"{a}-n{b}" for a, b in CASES])
def test_pack_nodes_equal_the_reference_tree(generic, name, which):
    P, eng = generic[name]
    n = _n_bits(P, which)
    n2 = P.N + 1 - n                                            # a second width in the same graph: 1 <-> N, 2 <-> N - 1
    x = random_glwe(0x9C00 + n, 4, P.glwe_len)
    x[3, ::5] = np.uint64((1 << 64) - 1)
    g = spf_amd.FheCircuit(eng)
    xi = [g.add_input(ValueKind.GLWE1, v) for v in x]
    one = g.add_trivial(ValueKind.GLWE1, 1)
    flipped = g.add_op(FheOp.Not, [xi[1]])
    added = g.add_op(FheOp.GlweAdd, [xi[2], xi[3]])
    value = {xi[0]: x[0], xi[1]: x[1], xi[2]: x[2], xi[3]: x[3], one: _trivial(1, P), flipped: _not(x[1], P),
             added: x[2] + x[3]}
    # level 0 (inputs, a constant) and level 1 (NOT, GlweAdd: two launches, two arena regions), in no arena order
    pool = [added, xi[0], one, flipped, xi[3], xi[2]]

    def rows_of(width, start):
        rows = [pool[(start + j) % len(pool)] for j in range(width)]
        if width > 1:
            rows[-1] = rows[0]                                  # one operand twice
        return rows

    rows1, rows2 = rows_of(n, 0), rows_of(n2, 3)
    p1 = g.add_pack(rows1)
    p2 = g.add_pack(rows2)
    np1 = g.add_op(FheOp.Not, [p1])                             # a pack node is an operand like any other ...
    rows3 = [np1, p1, xi[0]]
    p3 = g.add_pack(rows3)                                      # ... also of another pack
    outs = {node: g.add_output(node, ValueKind.GLWE1) for node in (p1, p2, np1, p3)}
    g.run()
    st = g.stats()
    # level 1: NOT + GlweAdd; level 2: the two packs, of different widths: two launches; level 3: NOT; level 4: pack
    assert st == {"nodes": 11, "levels": 4, "launches": 6}, st

    def expect(rows):
        vals = [value[r] for r in rows]
        tree = oracle_tree_pack(vals, P.N, P.k)
        assert np.array_equal(eng.glwe_pack(np.stack(vals)[None])[0], tree)
        return tree

    e1 = expect(rows1)
    assert np.array_equal(outs[p1], e1)
    assert np.array_equal(outs[p2], expect(rows2))
    value[p1], value[np1] = e1, _not(e1, P)
    assert np.array_equal(outs[np1], value[np1])
    assert np.array_equal(outs[p3], expect(rows3))
    g.close()


def test_unpack_of_sources_that_are_not_consecutive_gathers_one_row_per_integer(generic):
    """two inputs with another input between them, and a level-0 constant: one unpack group whose sources do not lie side
    by side, so they go through gather_rows_kernel first — one more launch than the consecutive case, whatever n_bits"""
    P, eng = generic["N32k2"]
    n = P.N - 1
    cts = random_glwe(0x9B40, 3, P.glwe_len)
    launches = {}
    for name, pick in (("consecutive", (0, 1)), ("apart", (2, 0))):
        g = spf_amd.FheCircuit(eng)
        ins = [g.add_input(ValueKind.GLWE1, x) for x in cts]
        one = g.add_trivial(ValueKind.GLWE1, 1)
        sources = [ins[pick[0]], ins[pick[1]]] + ([one] if name == "apart" else [])
        values = [cts[pick[0]], cts[pick[1]], _trivial(1, P)]
        outs = [[g.add_output(x, ValueKind.LWE1) for x in g.add_unpack(s, n)] for s in sources]
        g.run()
        st = g.stats()
        assert st["levels"] == 1 and st["nodes"] == 4 + len(sources) * n, st
        launches[name] = st["launches"]
        for s in range(len(sources)):
            for i in range(n):
                assert np.array_equal(outs[s][i], O.sample_extract(values[s], i, P.N, P.k)), (name, s, i)
        g.close()
    assert launches == {"consecutive": 1, "apart": 2}, launches


def test_recorded_circuit_with_packed_nodes_lowers_to_the_same_graph(generic):
    """`RecordedCircuit.lower` over unpack and pack nodes: the same node ids, the words of the graph built directly"""
    P, eng = generic["N16k1"]
    x = random_glwe(0x9C60, 2, P.glwe_len)

    def build(g):
        xi = [g.add_input(ValueKind.GLWE1, v) for v in x]
        bits = g.add_unpack(xi[0], 3)
        flipped = g.add_op(FheOp.Not, [xi[1]])
        packed = g.add_pack([xi[1], flipped, xi[0], flipped])
        more = g.add_unpack(packed, 2)
        return bits + more, packed

    rec = spf_amd.RecordedCircuit(P.N)
    lwes, packed = build(rec)
    for node in lwes:
        rec.add_output(node, ValueKind.LWE1)
    rec.add_output(packed, ValueKind.GLWE1)
    g, outs = rec.lower(eng)
    g.run()
    assert g.stats()["nodes"] == len(rec.op) == 2 + 3 + 1 + 1 + 2
    want_packed = oracle_tree_pack([x[1], _not(x[1], P), x[0], _not(x[1], P)], P.N, P.k)
    assert np.array_equal(outs[-1], want_packed)
    for i in range(3):
        assert np.array_equal(outs[i], O.sample_extract(x[0], i, P.N, P.k)), i
    for i in range(2):
        assert np.array_equal(outs[3 + i], O.sample_extract(want_packed, i, P.N, P.k)), i
    g.close()


def test_two_packs_of_one_width_are_one_launch(generic):
    P, eng = generic["N32k2"]
    x = random_glwe(0x9C40, 3, P.glwe_len)
    g = spf_amd.FheCircuit(eng)
    xi = [g.add_input(ValueKind.GLWE1, v) for v in x]
    rows = [[xi[0], xi[2], xi[1], xi[2], xi[0]], [xi[1], xi[1], xi[0], xi[2], xi[2]]]
    outs = [g.add_output(g.add_pack(r), ValueKind.GLWE1) for r in rows]
    g.run()
    assert g.stats() == {"nodes": 5, "levels": 1, "launches": 1}
    for r, o in zip(rows, outs):
        assert np.array_equal(o, oracle_tree_pack([x[i] for i in r], P.N, P.k))
    g.close()


def _decrypt_bits(glwe, ks, n):
    P = ks.params
    return np.array([O.decode(int(t), 1) for t in O.decrypt_glwe_raw(glwe, ks.glwe_sk, P.N, P.k)[:n]], dtype=np.uint64)


def _encrypt_packed(rng, ks, value, n):
    P = ks.params
    return O.encrypt_glwe(rng, ks.glwe_sk, spf_amd.packed_plaintext(value, n) << np.uint64(63), P.N, P.k, P.glwe_std)


def _round_trip_graph(eng, packed, n):
    """unpack -> KeyswitchL1toL0 -> CircuitBootstrap -> MultiplyGgswGlwe with the trivial one -> pack"""
    g = spf_amd.FheCircuit(eng)
    x = g.add_input(ValueKind.GLWE1, packed)
    one = g.add_trivial(ValueKind.GLWE1, 1)
    rows = []
    for b in g.add_unpack(x, n):
        sel = g.add_op(FheOp.CircuitBootstrap, [g.add_op(FheOp.KeyswitchL1toL0, [b])])
        rows.append(g.add_op(FheOp.MultiplyGgswGlwe, [sel, one]))
    return g, g.add_output(g.add_pack(rows), ValueKind.GLWE1)


@pytest.mark.parametrize("n,values", [(1, (1, 0)), (32, (0xDEADBEEF, 0x1234ABCD))], ids=["n1", "n32"])
def test_default128_packed_round_trip_decrypts(full, n, values):
    ks, eng = full
    rng = O.Rng(0x9D00 + n)
    packed = _encrypt_packed(rng, ks, values[0], n)
    g, out = _round_trip_graph(eng, packed, n)
    g.run()
    assert spf_amd.packed_decode(_decrypt_bits(out, ks, n), n, False) == values[0]
    st = g.stats()
    assert st["levels"] == 5 and st["launches"] == 5 and st["nodes"] == 2 + 4 * n + 1, st
    g._keep[0][...] = _encrypt_packed(rng, ks, values[1], n)    # the same graph on another input
    g.run()
    assert spf_amd.packed_decode(_decrypt_bits(out, ks, n), n, False) == values[1]
    g.close()


def _adder(g, ga, gb):
    """the ripple-carry CMUX chain of tests/test_gpu_graph.py over the selectors ga, gb -> (sum nodes, carry node)"""
    zero = g.add_trivial(ValueKind.GLWE1, 0)
    one = g.add_trivial(ValueKind.GLWE1, 1)
    carry = zero
    sums = []
    for i in range(len(ga)):
        ncarry = g.add_op(FheOp.Not, [carry])
        l1 = [g.add_op(FheOp.CMux, [gb[i], lo, hi]) for lo, hi in
              [(carry, ncarry), (ncarry, carry), (zero, carry), (carry, one)]]
        sums.append(g.add_op(FheOp.CMux, [ga[i], l1[0], l1[1]]))
        carry = g.add_op(FheOp.CMux, [ga[i], l1[2], l1[3]])
    return sums, carry


def _selectors(g, lwe1_nodes):
    return [g.add_op(FheOp.CircuitBootstrap, [g.add_op(FheOp.KeyswitchL1toL0, [x])]) for x in lwe1_nodes]


def test_encrypted_add_32_with_packed_io(full):
    ks, eng = full
    P = ks.params
    rng = O.Rng(0x9D40)
    a, b = 0xDEADBEEF, 0x1234ABCD
    # the bit-per-GLWE adder of tests/test_gpu_graph.py, for its counts
    plain = spf_amd.FheCircuit(eng)
    sel = []
    for bit in [(a >> i) & 1 for i in range(32)] + [(b >> i) & 1 for i in range(32)]:
        m = np.zeros(P.N, dtype=np.uint64)
        m[0] = O.encode(bit, 1)
        x = plain.add_input(ValueKind.GLWE1, O.encrypt_glwe(rng, ks.glwe_sk, m, P.N, P.k, P.glwe_std))
        sel.append(plain.add_op(FheOp.SampleExtract, [x], 0))
    sel = _selectors(plain, sel)
    sums, carry = _adder(plain, sel[:32], sel[32:])
    plain_outs = [plain.add_output(x, ValueKind.GLWE1) for x in sums + [carry]]
    plain.run()
    base = plain.stats()
    assert base["levels"] == 3 + 2 * 32 + 1
    got = sum(O.decode(int(O.decrypt_glwe_raw(o, ks.glwe_sk, P.N, P.k)[0]), 1) << i for i, o in enumerate(plain_outs))
    assert got == a + b
    plain.close()

    g = spf_amd.FheCircuit(eng)
    xa = g.add_input(ValueKind.GLWE1, _encrypt_packed(rng, ks, a, 32))
    xb = g.add_input(ValueKind.GLWE1, _encrypt_packed(rng, ks, b, 32))
    sel = _selectors(g, g.add_unpack(xa, 32) + g.add_unpack(xb, 32))
    sums, carry = _adder(g, sel[:32], sel[32:])
    out = g.add_output(g.add_pack(sums + [carry]), ValueKind.GLWE1)
    g.run()
    st = g.stats()
    assert st["levels"] == base["levels"] + 1, (st, base)               # the pack
    assert st["launches"] <= base["launches"] + 2, (st, base)           # the pack and one possible gather
    assert spf_amd.packed_decode(_decrypt_bits(out, ks, 33), 33, False) == a + b
    g._keep[0][...] = _encrypt_packed(rng, ks, 0xFFFFFFFF, 32)
    g._keep[1][...] = _encrypt_packed(rng, ks, 1, 32)
    g.run()
    assert spf_amd.packed_decode(_decrypt_bits(out, ks, 33), 33, False) == 0xFFFFFFFF + 1
    g.close()


def test_wrong_arguments_are_refused_and_the_graph_stays_usable(generic):
    import ctypes as C
    P, eng = generic["N16k1"]
    lib = eng._lib
    x = random_glwe(0x9E00, 1, P.glwe_len)[0]
    g = spf_amd.FheCircuit(eng)
    xi = g.add_input(ValueKind.GLWE1, x)
    lwe = g.add_input(ValueKind.LWE1, np.zeros(P.k * P.N + 1, dtype=np.uint64))
    bits = g.add_unpack(xi, 2)
    out = g.add_output(g.add_pack([xi, xi]), ValueKind.GLWE1)
    bit1 = g.add_output(bits[1], ValueKind.LWE1)
    want = oracle_tree_pack([x, x], P.N, P.k)
    n_nodes = g.stats()["nodes"]

    def still_runs():
        out[...] = 0
        g.run()
        assert np.array_equal(out, want) and np.array_equal(bit1, O.sample_extract(x, 1, P.N, P.k))
        assert g.stats()["nodes"] == n_nodes                      # a refused call added nothing

    still_runs()
    room = (C.c_uint32 * (P.N + 1))()
    two = (C.c_uint32 * 2)(xi, xi)
    many = (C.c_uint32 * (P.N + 1))(*([xi] * (P.N + 1)))
    node = C.c_uint32()
    raw = [
        ("unpack n_bits 0", lambda: lib.spf_graph_add_unpack(g._g, xi, 0, room)),
        ("unpack n_bits N + 1", lambda: lib.spf_graph_add_unpack(g._g, xi, P.N + 1, room)),
        ("unpack of no node", lambda: lib.spf_graph_add_unpack(g._g, 1234, 2, room)),
        ("unpack of an LWE", lambda: lib.spf_graph_add_unpack(g._g, lwe, 2, room)),
        ("unpack null out", lambda: lib.spf_graph_add_unpack(g._g, xi, 2, None)),
        ("unpack null graph", lambda: lib.spf_graph_add_unpack(None, xi, 2, room)),
        ("pack n_bits 0", lambda: lib.spf_graph_add_pack(g._g, two, 0, C.byref(node))),
        ("pack n_bits N + 1", lambda: lib.spf_graph_add_pack(g._g, many, P.N + 1, C.byref(node))),
        ("pack of no node", lambda: lib.spf_graph_add_pack(g._g, (C.c_uint32 * 2)(xi, 1234), 2, C.byref(node))),
        ("pack of an LWE", lambda: lib.spf_graph_add_pack(g._g, (C.c_uint32 * 2)(xi, bits[0]), 2, C.byref(node))),
        ("pack null nodes", lambda: lib.spf_graph_add_pack(g._g, None, 2, C.byref(node))),
        ("pack null out", lambda: lib.spf_graph_add_pack(g._g, two, 2, None)),
        ("pack null graph", lambda: lib.spf_graph_add_pack(None, two, 2, C.byref(node))),
    ]
    for what, call in raw:
        assert call() == 1, what                                  # SPF_ERR_INVALID_ARGUMENT
        still_runs()
    for what, call in [("unpack n_bits 0", lambda: g.add_unpack(xi, 0)), ("unpack n_bits N + 1", lambda: g.add_unpack(xi, P.N + 1)),
                       ("unpack of no node", lambda: g.add_unpack(1234, 2)), ("unpack of an LWE", lambda: g.add_unpack(lwe, 2)),
                       ("pack of nothing", lambda: g.add_pack([])), ("pack of N + 1", lambda: g.add_pack([xi] * (P.N + 1))),
                       ("pack of no node", lambda: g.add_pack([xi, 1234])), ("pack of an LWE", lambda: g.add_pack([bits[0]]))]:
        with pytest.raises(spf_amd.SpfError) as e:
            call()
        assert e.value.status == 1, what
        still_runs()
    g.close()


def test_group_jobs_with_packed_io_equal_one_context():
    """four jobs with packed input and output (the round trip through the circuit bootstrap at N = 16, widths 1, 2, 15, 16)
    dealt over a group [0, 0]: the words of a single-context run"""
    P = N16K1
    ks = O.gen_keyset(0x5EED0009, P)
    r = O.Rng(0x9E40)
    ak, ssk = O.gen_auto_key_fft(r, ks.glwe_sk, P), O.gen_ssk_fft(r, ks.glwe_sk, P)
    eng = spf_amd.Engine(_eng_params(P))
    grp = spf_amd.Group(_eng_params(P), devices=[0, 0])
    try:
        _load_all(eng, ks, ak, ssk)
        _load_all(grp, ks, ak, ssk)
        widths = [1, 2, 15, 16]
        packed = random_glwe(0x9E41, len(widths), P.glwe_len)
        jobs, outs = zip(*[_round_trip_graph(grp, packed[i], n) for i, n in enumerate(widths)])
        grp.run_graphs(list(jobs))
        assert sorted(j.member() for j in jobs) == [0, 0, 1, 1]
        for i, n in enumerate(widths):
            g1, o1 = _round_trip_graph(eng, packed[i], n)
            g1.run()
            assert np.array_equal(outs[i], o1) and o1.any(), n
            g1.close()
        first = [o.copy() for o in outs]
        grp.run_graphs(list(jobs))                                # the merged graphs again
        assert all(np.array_equal(u, v) for u, v in zip(first, outs))
        for j in jobs:
            j.close()
    finally:
        grp.close()
        eng.close()


def test_cpp_fhe_circuit_unpack_and_pack(tmp_path):
    """tests/cpp/packed_graph_parity.cpp, built and run as tests/test_gpu_packed.py builds packed_parity.cpp"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(spf_amd.lib_path())
    oracle_so = O.library_path()
    exe = tmp_path / "packed_graph_parity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(root, "include"),
                    "-I", os.path.join(root, "oracle"), os.path.join(root, "tests", "cpp", "packed_graph_parity.cpp"),
                    "-o", str(exe), "-L", libdir, "-lspf_hip", oracle_so,
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.dirname(oracle_so)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
