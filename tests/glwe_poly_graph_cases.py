"""Shared pieces of the tests of the plaintext polynomial linear maps over GLWE ciphertexts as gate-graph nodes
(`spf_graph_add_glwe_poly_linear`, include/spf_hip.h): the shapes, the slots, the operand pool of a layer, the graphs the tests
build, and the decrypt-level case with its plaintext model.  No tolerance anywhere: wrapping 64-bit integer arithmetic, words are
compared — against `poly_linear_ref` (tests/glwe_poly_cases.py) on the operand nodes' own words, against `Engine.glwe_poly_linear`
on the same rows, and against the oracle for the nodes around a layer."""
import numpy as np

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import glwe_poly_cases as GC
from tests.blind_rotation_graph_cases import packed_glwe
from tests.pbs_graph_cases import (CONTEXTS, NO_KEY, engine_params, keys_of, make_engine, same_words)  # noqa: F401
from tests.util import random_glwe

GLWE = ValueKind.GLWE1
LDS_ROWS, STREAM_ROWS = "glwe_poly_lds_rows_kernel", "glwe_poly_stream_rows_kernel"
BATCH_KERNELS = (GC.LDS, GC.STREAM)
VT = GC.row_tile()
# M below, at and over the rows of one workgroup (GLWE_POLY_VT = 4), K across the stream kernel's unroll of 4 and its remainder
SCATTERED_SHAPES = [(1, 1), (1, 5), (4, 4), (5, 7), (9, 2)]
LAYERS = 3       # grid.x > 1
SLOTS, MAX_ROWS = GC.SLOTS, GC.MAX_ROWS
INVALID = 1


def dims(P):
    return P.k + 1, P.N


def rows_kernel_name(triple, forced=None) -> str:
    """the kernel a graph whose operands do not lie consecutively must report under SPF_GLWE_POLY_PATH = forced (None: unset)"""
    return STREAM_ROWS if GC.is_constants_only(triple) and forced != "lds" else LDS_ROWS


def load(eng, slot, triple, M, K, bias=None):
    eng.load_glwe_poly_weights(slot, triple, bias, shape=(M, K))


def set_path(monkeypatch, path):
    if path is None:
        monkeypatch.delenv("SPF_GLWE_POLY_PATH", raising=False)
    else:
        monkeypatch.setenv("SPF_GLWE_POLY_PATH", path)


# ---- the slots of the scattered case ---------------------------------------------------------------------------------------------

def slots(M, K, N) -> dict:
    """name -> (CSR triple, bias or None) of an M x K matrix.  "general": exponents at every seam of `GC.seam_exponents`; polynomial
    (0, 0) holds every EXTREME_COEFFICIENT and an exponent three times over; where the shape has room: the first row tile is empty
    at k = K - 1 (its workgroups do not stage that operand), row 1 is empty altogether, and the second tile starts with an empty
    polynomial.  "constants": exponent 0 only (the stream kernel), with the same plants.  "empty": no term at all."""
    seams = GC.seam_exponents(N)

    def plant(polys, exps):
        cs = GC.EXTREME_COEFFICIENTS
        polys[0][0] = ([(exps[i % len(exps)], cs[i % len(cs)]) for i in range(max(len(exps), len(cs)))] +
                       [(exps[-1], GC.INT64_MAX), (exps[-1], GC.INT64_MAX), (exps[-1], 9)])
        if K >= 2:
            for m in range(min(VT, M)):
                polys[m][K - 1] = []
        if M >= 2:
            polys[1] = [[] for _ in range(K)]
        if M > VT:
            polys[VT][0] = []
        return GC.csr(polys, M, K)

    general = plant(GC.random_polys(0xA0, M, K, N, terms=3, cls="seams"), seams)
    constants = plant(GC.random_polys(0xA1, M, K, N, terms=2, cls="constants", empty_every=3), [0])
    empty = GC.csr([[[] for _ in range(K)] for _ in range(M)], M, K)
    assert set(general[1].tolist()) >= set(seams), "every seam exponent occurs"
    assert not GC.is_constants_only(general) and GC.is_constants_only(constants) and GC.is_constants_only(empty)
    bias = GC.random_bias(0xA2, M, N)
    return {"general+bias": (general, bias), "general": (general, None), "constants+bias": (constants, bias),
            "constants": (constants, None), "empty+bias": (empty, bias)}


# ---- the operand pool of a layer -------------------------------------------------------------------------------------------------

class GlwePool:
    """seven GLWE nodes of `g` from three levels, each an output so that the tests know its words: three inputs (0 .. 2), two XORs of
    inputs (3, 4: level 1, one group), and on level 2 a MulXN of the first XOR (5) and an XOR of the second with an input (6)"""

    def __init__(self, g, P, seed):
        self.P = P
        self.x = random_glwe(seed, 3, P.glwe_len)
        i = [g.add_input(GLWE, v) for v in self.x]
        a0, a1 = g.add_op(FheOp.GlweAdd, [i[0], i[1]]), g.add_op(FheOp.GlweAdd, [i[1], i[2]])
        self.nodes = i + [a0, a1, g.add_op(FheOp.MulXN, [a0], 3), g.add_op(FheOp.GlweAdd, [a1, i[0]])]
        self.outs = [g.add_output(n, GLWE) for n in self.nodes]

    def by_oracle(self) -> np.ndarray:
        P, x = self.P, self.x
        a0, a1 = O.glwe_xor(x[0], x[1], P.N, P.k), O.glwe_xor(x[1], x[2], P.N, P.k)
        return np.stack([x[0], x[1], x[2], a0, a1, O.glwe_mul_xn(a0, 3, P.N, P.k), O.glwe_xor(a1, x[0], P.N, P.k)])


def picks(layers, K) -> list:
    """indices into the pool of the K operands of every layer.  K >= 2: every layer starts with a node of the top level (so all
    layers stand on one level: one group), node 5 is shared by two layers, the last layer repeats its first operand, and the rest
    comes out of order from the two levels below.  K = 1: a lone row is consecutive by definition, so the single operands are the
    pool's inputs out of order — one level, one group, rows a whole GLWE apart and not ascending."""
    if K == 1:
        return [[1], [0], [2]][:layers]
    p = [[5 + o % 2] + [(2 * o + 3 * j) % 5 for j in range(1, K)] for o in range(layers)]
    p[-1][-1] = p[-1][0]
    return p


def pool_graph(eng, P, slot, layers, K, M, seed, with_layers=True):
    """-> (graph, pool, picks, [[output arrays of the M rows] per layer])"""
    g = spf_amd.FheCircuit(eng)
    pool = GlwePool(g, P, seed)
    pk = picks(layers, K)
    outs = [[g.add_output(n, GLWE) for n in g.add_glwe_poly_linear(slot, [pool.nodes[i] for i in p], M)] for p in pk] if with_layers else []
    return g, pool, pk, outs


def operand_rows(pool, pk, P) -> np.ndarray:
    """(layers, K, k+1, N): the operand nodes' own output words"""
    k1, N = dims(P)
    return np.stack([np.stack([pool.outs[i] for i in p]) for p in pk]).reshape(len(pk), len(pk[0]), k1, N)


def stack(outs, P) -> np.ndarray:
    k1, N = dims(P)
    return np.stack([np.stack(layer) for layer in outs]).reshape(len(outs), len(outs[0]), k1, N)


# ---- reload: one graph, four runs, other weights of the same shape before the last ---------------------------------------------------

def reload_rounds(eng, P):
    """a scattered layer (inputs, reversed) feeding an in-place one (its results), run three times on new contents, then once more
    after both slots were loaded again with other weights of the same shapes: every run gives the words of the weights loaded when
    it ran.  With SPF_GRAPH_CAPTURE=1 the second run captures and the third replays, so the reload falls after the capture."""
    k1, N = dims(P)
    K, M1, M2 = 3, VT + 1, 2
    x = random_glwe(0xA60, K, P.glwe_len)
    wa, ba = GC.csr(GC.random_polys(0xA61, M1, K, N, terms=2, cls="seams"), M1, K), GC.random_bias(0xA62, M1, N)
    wb, bb = GC.csr(GC.random_polys(0xA63, M2, M1, N, terms=2, cls="constants"), M2, M1), None
    load(eng, 4, wa, M1, K, ba)
    load(eng, 5, wb, M2, M1, bb)
    g = spf_amd.FheCircuit(eng)
    xs = [g.add_input(GLWE, row) for row in x]
    a = g.add_glwe_poly_linear(4, xs[::-1])
    b = g.add_glwe_poly_linear(5, a)
    out_a, out_b = [g.add_output(n, GLWE) for n in a], [g.add_output(n, GLWE) for n in b]
    for rnd in range(4):
        if rnd:
            x[...] = random_glwe(0xA60 + rnd, K, P.glwe_len)             # the same buffers, new contents
        if rnd == 3:
            wa, ba = GC.csr(GC.random_polys(0xA64, M1, K, N, terms=3, cls="mixed"), M1, K), None          # (loses its bias)
            wb, bb = GC.csr(GC.random_polys(0xA65, M2, M1, N, terms=2, cls="seams"), M2, M1), GC.random_bias(0xA66, M2, N)
            load(eng, 4, wa, M1, K, ba)                                  # (the constants-only slot becomes a general one)
            load(eng, 5, wb, M2, M1, bb)
        g.run()
        want_a = GC.poly_linear_ref(x[::-1].reshape(1, K, k1, N), wa, M1, K, ba)
        assert same_words(np.stack(out_a).reshape(want_a.shape), want_a), rnd
        want_b = GC.poly_linear_ref(want_a, wb, M2, M1, bb)
        assert same_words(np.stack(out_b).reshape(want_b.shape), want_b), rnd
    g.close()


# ---- the decrypt-level case (tuned context, the oracle's key set) -------------------------------------------------------------------
# Two packed 8-bit integers a and b, bit j at coefficient j with one plaintext bit (the message at 2^63): adding two such
# polynomials adds their bits modulo 2, and X^s moves bit j to coefficient j + s (no wrap: 8 + s <= N).  The slot is M = 1, K = 2,
# w = [X^s, 1]: the layer's GLWE carries the bits of (a << s) ^ b at coefficients 0 .. 8 + s, under the sum of the two noises.
BITS = 8
MODEL_CASES = [(0xB5, 0x6E, 3), (0xFF, 0x01, 0), (0x80, 0xFF, 5)]     # (a, b, s)


def model(a, b, s) -> list:
    """the bits of (a << s) ^ b, 8 + s of them"""
    v = (a << s) ^ b
    return [(v >> j) & 1 for j in range(BITS + s)]


def model_slot(s):
    return GC.csr([[[(s, 1)], [(0, 1)]]], 1, 2)


def model_encrypt(P, ks, a, b, seed=0xA70):
    rng = O.Rng(seed)
    return np.stack([packed_glwe(rng, ks.glwe_sk, P, a, BITS), packed_glwe(rng, ks.glwe_sk, P, b, BITS)])


def model_decrypt(ks, lwes) -> list:
    return [O.decode(O.decrypt_lwe_raw(row, ks.glwe_sk), 1) for row in lwes]
