"""The bootstraps by a caller's table and the public functional keyswitch as gate-graph nodes (`SPF_OP_PBS_UNIVARIATE`,
`SPF_OP_PBS_BIVARIATE`, `spf_graph_add_public_functional_keyswitch`, include/spf_hip.h), on the tuned DEFAULT_128 kernels and on
generic contexts at (N, k) = (128, 2) and (16, 1).  Every comparison is on words (tests/pbs_graph_cases.py `same_words`): against
the batch entry points on the same rows — themselves held to the oracle by test_gpu_bivariate.py, test_gpu_configs.py and
test_gpu_public_functional_keyswitch.py — and directly against the oracle.  One case decrypts."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import poly_ref as R
from tests import pbs_graph_cases as K
from tests import pufks_cases as PC
from tests.polyref_cases import key_fft
from tests.util import random_glwe, random_lwe_batch, to_engine_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(which):
        if which not in made:
            made[which] = K.make_engine(which)
        return K.keys_of(which)[0], made[which], K.keys_of(which)[1]

    yield get
    for e in made.values():
        e.close()


def run_and_close(g):
    g.run()
    st = g.stats()
    g.close()
    return st


# ---- the two bootstraps ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("which", K.CONTEXTS)
def test_univariate_nodes_one_table_or_one_per_node(rigs, which, B):
    P, eng, ks = rigs(which)
    x, luts = random_lwe_batch(0xE00 + B, B, P.lwe_n), random_glwe(0xE01 + B, B, P.glwe_len)

    def graph(shared):
        g = spf_amd.FheCircuit(eng)
        t = [g.add_input(ValueKind.GLWE1, v) for v in (luts[:1] if shared else luts[::-1])]   # (distinct tables: not in node order)
        xs = [g.add_input(ValueKind.LWE0, v) for v in x]
        outs = [g.add_output(g.add_op(FheOp.PBS_UNIVARIATE, [xs[i], t[0] if shared else t[B - 1 - i]], 77), ValueKind.LWE1)
                for i in range(B)]
        return run_and_close(g), np.stack(outs)

    # (input LWEs start at multiples of 256 bytes: more than one of them is gathered, in either graph)
    st, got = graph(True)
    assert st == {"nodes": 1 + 2 * B, "levels": 1, "launches": 1 + (B > 1)}, st   # one table node: read in place, ONE launch
    assert K.same_words(got, eng.pbs_univariate(x, luts[0]))
    st2, got2 = graph(False)
    assert st2 == {"nodes": 3 * B, "levels": 1, "launches": st["launches"] + (B > 1)}, st2   # ... and the tables gathered
    assert K.same_words(got2, eng.pbs_univariate(x, luts))
    assert K.same_words(got2[0], got[0])
    for i in sorted({0, B - 1}):
        assert K.same_words(got2[i], O.pbs_univariate(x[i], luts[i], ks.bsk_fft, P)), i


@pytest.mark.parametrize("which", K.CONTEXTS)
def test_a_computed_table_and_operands_from_two_levels(rigs, which):
    """the table is MUL_XN of an input, the LWEs an input and a keyswitch result: both operands of the group are gathered"""
    P, eng, ks = rigs(which)
    x0, l1, lut = random_lwe_batch(0xE10, 1, P.lwe_n)[0], random_lwe_batch(0xE11, 1, P.k * P.N)[0], random_glwe(0xE12, 1, P.glwe_len)[0]
    g = spf_amd.FheCircuit(eng)
    t = g.add_op(FheOp.MulXN, [g.add_input(ValueKind.GLWE1, lut)], 5)
    a = g.add_input(ValueKind.LWE0, x0)
    b = g.add_op(FheOp.KeyswitchL1toL0, [g.add_input(ValueKind.LWE1, l1)])
    outs = [g.add_output(g.add_op(FheOp.PBS_UNIVARIATE, [n, t]), ValueKind.LWE1) for n in (b, a)]
    biv = g.add_output(g.add_op(FheOp.PBS_BIVARIATE, [b, a, t], 1), ValueKind.LWE1)
    st = run_and_close(g)
    # MUL_XN, keyswitch | gather of the two LWEs + univariate launch, lwe_pack_kernel + bivariate launch
    assert st == {"nodes": 8, "levels": 2, "launches": 6}, st
    t_want = O.glwe_mul_xn(lut, 5, P.N, P.k)
    b_want = O.keyswitch_lwe(l1, ks.ksk, P.k * P.N, P.lwe_n, P.ks_radix_log, P.ks_count)
    assert K.same_words(outs[0], O.pbs_univariate(b_want, t_want, ks.bsk_fft, P))
    assert K.same_words(outs[1], O.pbs_univariate(x0, t_want, ks.bsk_fft, P))
    assert K.same_words(biv, O.pbs_univariate(K.pack(b_want, x0, 1), t_want, ks.bsk_fft, P))
    assert K.same_words(np.stack(outs), eng.pbs_univariate(np.stack([b_want, x0]), t_want))


BIVARIATE = [(w, p, B) for w in K.CONTEXTS for p in (0, 2, 63) for B in (1, 5)] + [("n16k1", 2, 257)]


@pytest.mark.parametrize("which,p,B", BIVARIATE, ids=[f"{w}-p{p}-B{B}" for w, p, B in BIVARIATE])
def test_bivariate_nodes(rigs, which, p, B):
    """f(x, x) on one node twice, and left / right in another order than the nodes: input LWEs do not lie consecutively, so from
    B = 2 on lwe_pack_rows_kernel reads them where they lie (at B = 257 its grid-stride loop runs).  Keyswitch results do lie
    consecutively: they keep lwe_pack_kernel."""
    P, eng, ks = rigs(which)
    x, lut = random_lwe_batch(0xE20 + B, B, P.lwe_n), random_glwe(0xE21 + p, 1, P.glwe_len)[0]
    l1 = random_lwe_batch(0xE22 + B, B, P.k * P.N)
    right = [(3 * i + 1) % B for i in range(B)]
    g = spf_amd.FheCircuit(eng)
    t = g.add_input(ValueKind.GLWE1, lut)
    xs = [g.add_input(ValueKind.LWE0, v) for v in x]
    same = [g.add_output(g.add_op(FheOp.PBS_BIVARIATE, [n, n, t], p), ValueKind.LWE1) for n in xs]
    c = spf_amd.FheCircuit(eng)
    t = c.add_input(ValueKind.GLWE1, lut)
    l0 = [c.add_op(FheOp.KeyswitchL1toL0, [c.add_input(ValueKind.LWE1, v)]) for v in l1]
    consecutive = [c.add_output(c.add_op(FheOp.PBS_BIVARIATE, [n, n, t], p), ValueKind.LWE1) for n in l0]
    assert run_and_close(c) == {"nodes": 1 + 3 * B, "levels": 2, "launches": 1 + (B > 1) + 2}   # (gather,) keyswitch, pack, bootstrap
    l0_want = eng.keyswitch_lwe_l1_lwe_l0(l1)
    assert K.same_words(np.stack(consecutive), eng.pbs_bivariate(l0_want, l0_want, lut, p))
    h = spf_amd.FheCircuit(eng)
    t = h.add_input(ValueKind.GLWE1, lut)
    xs = [h.add_input(ValueKind.LWE0, v) for v in x]
    mixed = [h.add_output(h.add_op(FheOp.PBS_BIVARIATE, [xs[B - 1 - i], xs[right[i]], t], p), ValueKind.LWE1) for i in range(B)]
    assert run_and_close(g) == {"nodes": 1 + 2 * B, "levels": 1, "launches": 2}
    assert run_and_close(h) == {"nodes": 1 + 2 * B, "levels": 1, "launches": 2}
    assert K.same_words(np.stack(same), eng.pbs_bivariate(x, x, lut, p))
    assert K.same_words(np.stack(mixed), eng.pbs_bivariate(x[::-1], x[right], lut, p))
    for i in sorted({0, B - 1}):
        assert K.same_words(mixed[i], O.pbs_univariate(K.pack(x[B - 1 - i], x[right[i]], p), lut, ks.bsk_fft, P)), i


# ---- the public functional keyswitch ----------------------------------------------------------------------------------------

def pufks_graph(eng, P, kind, outputs, count, seed, contiguous=False):
    """`outputs` keyswitch nodes of `count` rows each from the six-node pool (or, contiguous, from inputs in row order); each an
    output and the source of an unpack.  -> (stats, rows (outputs, count, n + 1), GLWEs, [unpacked LWEs of node 0])"""
    g = spf_amd.FheCircuit(eng)
    if contiguous:   # the rows of one unpack group (and of the keyswitch group behind it), in their own order
        ids = [g.add_unpack(g.add_input(ValueKind.GLWE1, v), count) for v in random_glwe(seed, outputs, P.glwe_len)]
        if ValueKind(kind) == ValueKind.LWE0:
            ids = [[g.add_op(FheOp.KeyswitchL1toL0, [b]) for b in x] for x in ids]
        row_outs = [[g.add_output(n, kind) for n in x] for x in ids]
    else:
        pool = K.RowPool(g, P, kind, seed)
        picks = [pool.pick(o, count) for o in range(outputs)]
        ids = [[pool.nodes[i] for i in pk] for pk in picks]
        n_other = g.stats()["nodes"]
    nodes = [g.add_public_functional_keyswitch(x) for x in ids]
    outs = [g.add_output(n, ValueKind.GLWE1) for n in nodes]
    bits = [g.add_output(b, ValueKind.LWE1) for b in g.add_unpack(nodes[0], min(count, 3))]
    g.run()
    st = g.stats()
    g.close()
    if contiguous:
        rows = np.stack([np.stack(x) for x in row_outs])
    else:
        rows = np.stack([np.stack([pool.outs[i] for i in pk]) for pk in picks])
        assert st["nodes"] == n_other + outputs + min(count, 3)
    return st, rows, np.stack(outs), bits


@pytest.mark.parametrize("kind", [ValueKind.LWE0, ValueKind.LWE1], ids=["lwe0", "lwe1"])
@pytest.mark.parametrize("which", K.CONTEXTS)
def test_keyswitch_nodes_at_the_tile_edges(rigs, which, kind):
    P, eng, ks = rigs(which)
    n, count = K.dimension(P, kind), 4 if which == "tuned" else 3
    key = K.pufks_key(P.N, P.k, n, count)
    eng.load_public_functional_keyswitch_key_std(key, 4, count)
    keyf = key_fft(key) if n <= 64 else None                     # (the oracle itself: where it is a matter of milliseconds)
    for outputs in (1, 3):
        for lwe_count in (1, 31, 32, 33):
            if lwe_count > P.N:
                continue
            st, rows, got, bits = pufks_graph(eng, P, kind, outputs, lwe_count, 0xE30 + lwe_count)
            want = eng.public_functional_keyswitch(rows)
            assert K.same_words(got, want), (outputs, lwe_count)
            for i, b in enumerate(bits):
                assert K.same_words(b, O.sample_extract(want[0], i, P.N, P.k)), (outputs, lwe_count, i)
            if keyf is not None:
                assert K.same_words(got[-1], PC.pufks_oracle(rows[-1], keyf, P.N, P.k, 4, count).reshape(-1)), (outputs, lwe_count)
    # rows that happen to lie consecutively take the contiguous entry point: no gather, no pointer table
    st, rows, got, _ = pufks_graph(eng, P, kind, 3, min(33, P.N), 0xE3F, contiguous=True)
    # unpack (, keyswitch), (pre-pass +) main launch, the unpack of node 0
    assert st["launches"] == 1 + (kind == ValueKind.LWE0) + (2 if which == "tuned" else 1) + 1, st
    assert K.same_words(got, eng.public_functional_keyswitch(rows))


@pytest.mark.parametrize("log,count,kernel", [(4, 8, "pufks4_kernel<4,8>"), (4, 4, "pufks4_kernel<4,4>"), (5, 3, "generic_pufks_kernel")])
def test_keyswitch_nodes_at_every_radix_family_of_the_tuned_context(rigs, log, count, kernel):
    P, eng, ks = rigs("tuned")
    key = K.pufks_key(P.N, P.k, P.lwe_n, count, seed=log)
    eng.load_public_functional_keyswitch_key_std(key, log, count)
    keyf = key_fft(key)
    st, rows, got, _ = pufks_graph(eng, P, ValueKind.LWE0, 3, 33, 0xE40 + count)
    assert eng.last_public_functional_keyswitch_kernel() == kernel
    # keyswitches, sample extracts and their gathers aside: pre-pass + main launch, or gather + generic launch; then the unpack
    assert K.same_words(got, eng.public_functional_keyswitch(rows))
    for o in range(3):
        assert K.same_words(got[o], PC.pufks_oracle(rows[o], keyf, P.N, P.k, log, count).reshape(-1)), o


def test_keyswitch_node_from_level0_rows_of_dimension_637():
    """from_dimension = 637 is no multiple of the pre-pass tile; no bootstrap here, so no bootstrap key: uniform keyswitch keys"""
    P = O.DEFAULT_128
    eng = spf_amd.Engine(to_engine_params(P))
    try:
        rng = np.random.default_rng(0xE50)
        eng.load_keyswitch_key(rng.integers(0, 1 << 64, P.k * P.N * P.ks_count * (P.lwe_n + 1), dtype=np.uint64))
        eng.load_public_functional_keyswitch_key_std(K.pufks_key(P.N, P.k, P.lwe_n, 4), 4, 4)
        for outputs, lwe_count in ((1, 33), (3, 7)):
            st, rows, got, _ = pufks_graph(eng, P, ValueKind.LWE0, outputs, lwe_count, 0xE51)
            assert rows.shape == (outputs, lwe_count, 638)
            assert K.same_words(got, eng.public_functional_keyswitch(rows)), (outputs, lwe_count)
    finally:
        eng.close()


def test_bad_arguments_are_refused_and_the_graph_stays_usable(rigs):
    P, eng, ks = rigs("tuned")
    g = spf_amd.FheCircuit(eng)
    a = g.add_input(ValueKind.LWE0, random_lwe_batch(0xE60, 1, P.lwe_n)[0])
    l1 = g.add_input(ValueKind.LWE1, random_lwe_batch(0xE61, 1, P.k * P.N)[0])
    lut = g.add_input(ValueKind.GLWE1, random_glwe(0xE62, 1, P.glwe_len)[0])
    lib, n_nodes = eng._lib, g.stats()["nodes"]
    node = C.c_uint32(77)
    many = (C.c_uint32 * (P.N + 1))(*([a] * (P.N + 1)))

    def refused(status_call, word):
        assert status_call() == 1
        assert word in lib.spf_last_error(eng._h).decode(), lib.spf_last_error(eng._h)
        assert g.stats()["nodes"] == n_nodes and node.value == 77      # nothing recorded

    add = lib.spf_graph_add_public_functional_keyswitch
    refused(lambda: add(g._g, many, 0, C.byref(node)), "lwe_count")
    refused(lambda: add(g._g, many, P.N + 1, C.byref(node)), "lwe_count")
    refused(lambda: add(g._g, (C.c_uint32 * 2)(a, l1), 2, C.byref(node)), "mixed")
    refused(lambda: add(g._g, (C.c_uint32 * 2)(l1, a), 2, C.byref(node)), "mixed")
    refused(lambda: add(g._g, (C.c_uint32 * 2)(a, lut), 2, C.byref(node)), "not an LWE")
    refused(lambda: add(g._g, (C.c_uint32 * 2)(a, n_nodes), 2, C.byref(node)), "not a node")
    refused(lambda: add(g._g, None, 2, C.byref(node)), "null")
    refused(lambda: add(g._g, many, 2, None), "null")
    assert add(None, many, 2, C.byref(node)) == 1
    op = lib.spf_graph_add_op
    refused(lambda: op(g._g, int(FheOp.PBS_BIVARIATE), (C.c_uint32 * 3)(a, a, lut), 3, 64, C.byref(node)), "plaintext_bits")
    refused(lambda: op(g._g, int(FheOp.PBS_BIVARIATE), (C.c_uint32 * 3)(a, a, lut), 2, 0, C.byref(node)), "number of operands")
    refused(lambda: op(g._g, int(FheOp.PBS_UNIVARIATE), (C.c_uint32 * 3)(a, a, lut), 3, 0, C.byref(node)), "number of operands")
    refused(lambda: op(g._g, int(FheOp.PBS_UNIVARIATE), (C.c_uint32 * 2)(l1, lut), 2, 0, C.byref(node)), "wrong ciphertext type")
    refused(lambda: op(g._g, int(FheOp.PBS_BIVARIATE), (C.c_uint32 * 3)(a, lut, lut), 3, 0, C.byref(node)), "wrong ciphertext type")
    refused(lambda: op(g._g, 12, (C.c_uint32 * 2)(a, lut), 2, 0, C.byref(node)), "unknown operation")
    with pytest.raises(spf_amd.SpfError, match="lwe_count"):
        g.add_public_functional_keyswitch([])
    assert g.add_public_functional_keyswitch([a] * P.N) == n_nodes             # lwe_count = N: accepted
    g.close()


def test_errors_of_the_run_and_the_graph_still_runs_once_the_key_is_there():
    P, ks = K.keys_of("tuned")[:2]
    eng = spf_amd.Engine(K.engine_params(P))
    try:
        rows = random_lwe_batch(0xE70, 3, P.lwe_n)
        g = spf_amd.FheCircuit(eng)
        out = g.add_output(g.add_public_functional_keyswitch([g.add_input(ValueKind.LWE0, rows[i]) for i in (2, 0, 1)]), ValueKind.GLWE1)
        with pytest.raises(spf_amd.SpfError) as e:
            g.run()
        assert e.value.status == K.NO_KEY and "public functional keyswitch key" in str(e.value)
        eng.load_public_functional_keyswitch_key_std(K.pufks_key(P.N, P.k, P.lwe_n + 1, 4), 4, 4)
        with pytest.raises(spf_amd.SpfError) as e:
            g.run()
        assert e.value.status == 1 and str(P.lwe_n + 1) in str(e.value) and f" {P.lwe_n} " in str(e.value), str(e.value)
        h, out_h = None, None
        for log, count in ((4, 4), (5, 3), (4, 8)):        # a hand-written radix, then the generic kernel (which gathers), then back
            eng.load_public_functional_keyswitch_key_std(K.pufks_key(P.N, P.k, P.lwe_n, count, seed=log), log, count)
            if h is None:                                   # a second graph, first planned under the hand-written radix
                h = spf_amd.FheCircuit(eng)
                out_h = h.add_output(h.add_public_functional_keyswitch([h.add_input(ValueKind.LWE0, rows[i]) for i in (2, 0, 1)]),
                                     ValueKind.GLWE1)
            g.run()
            h.run()
            want = eng.public_functional_keyswitch(rows[[2, 0, 1]][None])[0]
            assert K.same_words(out, want) and K.same_words(out_h, want), (log, count)
        g.close()
        h.close()
    finally:
        eng.close()


# ---- whole graphs -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", K.CONTEXTS)
def test_one_chain_mixing_everything_run_twice(rigs, which):
    P, eng, ks = rigs(which)
    W, p, count = 3, 2, 4 if which == "tuned" else 3
    eng.load_public_functional_keyswitch_key_std(K.pufks_key(P.N, P.k, P.k * P.N, count), 4, count)
    glwe, lut = random_glwe(0xE80, 2, P.glwe_len), random_glwe(0xE81, 1, P.glwe_len)[0]
    x = glwe[0].copy()
    g = spf_amd.FheCircuit(eng)
    outs = K.mixed_chain(g, x, lut, W, p)
    for run in range(2):
        x[...] = glwe[run]                                  # the second run: new contents of the input, the same graph
        g.run()
        want = K.mixed_chain_by_batch_calls(eng, glwe[run], lut, W, p)
        for name in ("l0", "biv", "packed", "sel", "out"):
            assert K.same_words(np.stack(outs[name]) if isinstance(outs[name], list) else outs[name], want[name]), (run, name)
    # unpack | keyswitch | rows packed + bivariate | pre-pass + keyswitch (generic: + gather), circuit bootstrap | cmux
    st = g.stats()
    assert st["nodes"] == 2 + 3 * W + 3 and st["levels"] == 5, st
    g.close()
    sel = O.circuit_bootstrap(want["l0"][0], ks.bsk_fft, K.keys_of(which)[2], K.keys_of(which)[3], P)
    assert K.same_words(want["sel"], sel)
    assert K.same_words(want["out"], O.cmux(want["packed"], glwe[1], sel, P.N, P.k, P.cbs_radix_log, P.cbs_count))


def decode_with_carry(d: int, p: int, c: int) -> int:
    """`decrypt_lwe_with_carry` (high_level.rs:586-611) after the raw decryption"""
    round_bit = (d >> (64 - p - c - 1)) & 1
    return ((d >> (64 - p - c)) + round_bit) & ((1 << p) - 1)


def test_digits_added_by_a_bivariate_table_and_packed_decrypt_at_default128():
    """2-bit digits l + r mod 4 through a bivariate table, the sums keyswitched to level 0 and packed by the public functional
    keyswitch under an honest key (pufks_cases.honest_key): coefficient j of the packed GLWE carries the phase of sum j within
    pufks_cases.meaning_bounds, nothing beyond the last one, and decodes to the digit"""
    P = O.DEFAULT_128.replace(lwe_n=32)
    ks = O.gen_keyset(0x5EED0021, P)
    count, log, p, c = 4, 4, 2, 2
    key = PC.honest_key(np.random.default_rng(0xE90), ks.lwe_sk, ks.glwe_sk, P.N, log, count)
    eng = spf_amd.Engine(to_engine_params(P))
    try:
        eng.load_bootstrap_key(ks.bsk_fft)
        eng.load_keyswitch_key(ks.ksk)
        eng.load_public_functional_keyswitch_key_std(key, log, count)
        rng = O.Rng(0xE91)
        pairs = [(l, r) for l in range(4) for r in range(4)]
        enc = lambda m: O.encrypt_lwe(rng, ks.lwe_sk, m << (64 - p - c - 1), P.lwe_std)  # noqa: E731
        g = spf_amd.FheCircuit(eng)
        t = g.add_input(ValueKind.GLWE1, spf_amd.generate_bivariate_lut(lambda l, r: (l + r) % 4, p, c))
        sums = [g.add_op(FheOp.KeyswitchL1toL0, [g.add_op(FheOp.PBS_BIVARIATE, [g.add_input(ValueKind.LWE0, enc(l)),
                                                                                g.add_input(ValueKind.LWE0, enc(r)), t], p)])
                for l, r in pairs]
        rows = [g.add_output(n, ValueKind.LWE0) for n in sums]
        out = g.add_output(g.add_public_functional_keyswitch(sums), ValueKind.GLWE1)
        g.run()
        g.close()
    finally:
        eng.close()
    PC.check_meaning(out.reshape(P.k + 1, P.N), np.stack(rows), ks.lwe_sk, ks.glwe_sk, count, log, "graph")
    phase = R.glwe_phase(out.reshape(P.k + 1, P.N), ks.glwe_sk)
    assert [decode_with_carry(int(phase[j]), p, c) for j in range(len(pairs))] == [(l + r) % 4 for l, r in pairs]


def test_recorded_circuit_lowers_to_the_same_words(rigs):
    P, eng, ks = rigs("n128k2")
    eng.load_public_functional_keyswitch_key_std(K.pufks_key(P.N, P.k, P.k * P.N, 3), 4, 3)
    glwe, lut = random_glwe(0xEA0, 1, P.glwe_len)[0], random_glwe(0xEA1, 1, P.glwe_len)[0]
    rec = spf_amd.RecordedCircuit(P.N)
    K.mixed_chain(rec, glwe, lut, 3, 2)
    g, outs = rec.lower(eng)
    g.run()
    g.close()
    want = K.mixed_chain_by_batch_calls(eng, glwe, lut, 3, 2)
    assert K.same_words(outs[-1], want["out"]) and K.same_words(outs[-3], want["packed"])
    a = rec.arrays()
    again = spf_amd.RecordedCircuit.from_arrays(a, rec.kind, rec.host, P.N)
    assert again.op == rec.op and again.param == rec.param and again.inputs == rec.inputs


def test_group_jobs_carry_the_new_nodes_through_a_merge(rigs):
    """two jobs over members [0, 0] — whichever way they are dealt, the words are one context's"""
    P, eng, ks = rigs("tuned")
    W, p = 3, 2
    key = K.pufks_key(P.N, P.k, P.k * P.N, 4)
    eng.load_public_functional_keyswitch_key_std(key, 4, 4)
    glwe, lut = random_glwe(0xEB0, 2, P.glwe_len), random_glwe(0xEB1, 1, P.glwe_len)[0]
    grp = spf_amd.Group(K.engine_params(P), devices=[0, 0])
    jobs = []
    try:
        K.load_keys(grp, "tuned")
        grp.load_public_functional_keyswitch_key_std(key, 4, 4)
        for j in range(2):
            g = spf_amd.FheCircuit(grp)
            jobs.append((g, K.mixed_chain(g, glwe[j], lut, W, p)))
        grp.run_graphs([g for g, _ in jobs])
        for j, (_, outs) in enumerate(jobs):
            want = K.mixed_chain_by_batch_calls(eng, glwe[j], lut, W, p)
            assert K.same_words(outs["packed"], want["packed"]) and K.same_words(outs["out"], want["out"]), j
            assert K.same_words(np.stack(outs["biv"]), want["biv"]), j
    finally:
        for g, _ in jobs:
            g.close()
        grp.close()
