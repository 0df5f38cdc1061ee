"""Shared pieces of the tests of the plaintext linear maps over LWE ciphertexts as gate-graph nodes (`spf_graph_add_lwe_linear`,
include/spf_hip.h): the shapes, the weights, the graphs the tests build, the chain "layer -> table -> layer -> table" with its
walk by the oracle, and the plaintext model of the decrypt-level case.  No tolerance anywhere: integer arithmetic, words are
compared — against `linear_ref` (tests/lwe_linear_cases.py) on the operand nodes' own words, against `Engine.lwe_linear` on the
same rows, and against the oracle for the nodes around the linear node."""
import numpy as np

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests import lwe_linear_cases as LC
from tests.pbs_graph_cases import (CONTEXTS, NO_KEY, RowPool, dimension, engine_params, keys_of, make_engine,  # noqa: F401
                                   pufks_key, same_words)
from tests.util import random_glwe, random_lwe_batch

ROWS_KERNEL = "lwe_linear_rows_kernel"
BATCH_KERNELS = (LC.VALU, "pfks_gemm_kernel<1>", "pfks_gemm_kernel<2>", "pfks_gemm_kernel<3>")
KINDS = [ValueKind.LWE0, ValueKind.LWE1]
# M below, at and above the rows of one workgroup (LWE_LINEAR_VT = 8), K off the unroll factor (4)
SCATTERED_SHAPES = [(1, 1), (1, 5), (8, 4), (9, 7), (17, 3)]
LAYERS = 3      # more than one workgroup along grid.x; the picks of three layers never lie consecutively, whatever K
MAX_ROWS = 4096  # SPF_GRAPH_LWE_LINEAR_MAX_ROWS
SLOTS = 64       # SPF_LWE_LINEAR_SLOTS

# weights no limb image holds, next to the small ones (the VALU product reads the int64 matrix)
HARD_WEIGHTS = np.array([[LC.INT64_MIN, LC.INT64_MAX, -1, 0],
                         [1, LC.FIRST_BEYOND[0], LC.FIRST_BEYOND[1], LC.INT64_MIN],
                         [0, 1, LC.INT64_MAX, -1]], dtype=np.int64)


def words(P, kind) -> int:
    return dimension(P, kind) + 1


def weights(seed, M, K, bias: bool):
    """an (M, K) matrix of two-limb weights with both ends of the class planted, and M uniform bias words or None"""
    w = LC.class_weights(seed, M, K, 2)
    b = np.random.default_rng([0xE3, seed, M]).integers(0, 1 << 64, M, dtype=np.uint64) if bias else None
    return w, b


def load_pool_key(eng, which, P, kind):
    """RowPool's LWE0 rows pass through a public functional keyswitch: it needs a key of the LWE0 dimension"""
    if ValueKind(kind) == ValueKind.LWE0:
        count = 4 if which == "tuned" else 3
        eng.load_public_functional_keyswitch_key_std(pufks_key(P.N, P.k, P.lwe_n, count), 4, count)


def pool_graph(eng, P, kind, slot, layers, K, M, seed):
    """`layers` linear nodes of K operands each, picked from the six-node pool (three levels, repeats from the seventh on).
    K = 1: a layer's level is its operand's, a layer alone on its level is its own group, and ONE row lies consecutively by
    definition (the in-place path, rightly) — so the single operands are the pool's two inputs, [1], [0], [1], ...: one level, one
    group, rows 256 bytes apart and out of order.
    -> (graph, rows (layers, K, W) once it ran, [[output arrays of the M rows] per layer])"""
    g = spf_amd.FheCircuit(eng)
    pool = RowPool(g, P, kind, seed)
    picks = [pool.pick(o, K) for o in range(layers)] if K > 1 else [[(o + 1) % 2] for o in range(layers)]
    outs = [[g.add_output(n, kind) for n in g.add_lwe_linear(slot, [pool.nodes[i] for i in pk], M)] for pk in picks]
    return g, (lambda: np.stack([np.stack([pool.outs[i] for i in pk]) for pk in picks])), outs


def stack(outs) -> np.ndarray:
    return np.stack([np.stack(layer) for layer in outs])


def input_rows(g, kind, rows):
    """one input node per row, each also an output -> (nodes, output arrays)"""
    nodes = [g.add_input(kind, r) for r in rows]
    return nodes, [g.add_output(n, kind) for n in nodes]


# ---- the chain: inputs -> linear A -> (keyswitch, lwe1 only) -> table 1 -> linear B -> keyswitch -> table 2 -> outputs ------------
# (a bootstrap by table takes a level-0 LWE and gives a level-1 one: the second layer works on the first table's results where they
# lie, and its rows are keyswitched for the second table)

def chain(g, kind, slot_a, slot_b, x, lut1, lut2, M1, M2):
    """`x`: (K, W) array whose rows are the inputs (read at every run) -> {stage: [output arrays]}"""
    kind = ValueKind(kind)
    t1, t2 = g.add_input(ValueKind.GLWE1, lut1), g.add_input(ValueKind.GLWE1, lut2)
    xs = [g.add_input(kind, row) for row in x]
    a = g.add_lwe_linear(slot_a, xs, M1)
    a0 = [g.add_op(FheOp.KeyswitchL1toL0, [n]) for n in a] if kind == ValueKind.LWE1 else a
    h = [g.add_op(FheOp.PBS_UNIVARIATE, [n, t1]) for n in a0]
    b = g.add_lwe_linear(slot_b, h, M2)
    b0 = [g.add_op(FheOp.KeyswitchL1toL0, [n]) for n in b]
    y = [g.add_op(FheOp.PBS_UNIVARIATE, [n, t2]) for n in b0]
    return {"a": [g.add_output(n, kind) for n in a], "h": [g.add_output(n, ValueKind.LWE1) for n in h],
            "b": [g.add_output(n, ValueKind.LWE1) for n in b], "y": [g.add_output(n, ValueKind.LWE1) for n in y]}


def chain_by_oracle(P, ks, kind, x, wa, ba, wb, bb, lut1, lut2):
    """the same steps: `linear_ref` for the layers, the oracle's keyswitch and univariate bootstrap around them"""
    def keyswitch(rows):
        return np.stack([O.keyswitch_lwe(r, ks.ksk, P.k * P.N, P.lwe_n, P.ks_radix_log, P.ks_count) for r in rows])

    def table(rows, lut):
        return np.stack([O.pbs_univariate(r, lut, ks.bsk_fft, P) for r in rows])

    a = LC.linear_ref(x, wa, ba)
    h = table(keyswitch(a) if ValueKind(kind) == ValueKind.LWE1 else a, lut1)
    b = LC.linear_ref(h, wb, bb)
    return {"a": a, "h": h, "b": b, "y": table(keyswitch(b), lut2)}


# ---- the decrypt-level case (tuned context, level-0 inputs) ---------------------------------------------------------------------
# A table over `bits` plaintext bits reads its message at 2^(63 - bits) (one padding bit above it) and writes f at 2^(64 - bits)
# (`generate_lut`: delta = 64 - bits), so a result of a 3-bit table is a message of a 2-bit one: layer A lives in 3 bits, layer B
# in 2.  The keyswitch before table 2 adds ~2^-6.7 of the torus (2048 * 6 digits of a radix-4 key at lwe_std): a 2-bit slot is
# 2^-4 wide on each side, a 3-bit one would be 2^-5.  Weights in {-1, 0, 1, 2}, K = 4 -> M = 3 -> M = 2, every pre-activation
# inside its plaintext space for both input vectors.
BITS_A, BITS_B = 3, 2
MODEL_WA = np.array([[1, 1, 0, 0], [2, -1, 1, 0], [0, 1, -1, 2]], dtype=np.int64)
MODEL_BIAS_A = [1, 0, 2]
MODEL_WB = np.array([[1, 0, 1], [2, -1, 0]], dtype=np.int64)
MODEL_INPUTS = [[1, 2, 1, 1], [2, 1, 1, 0]]


def model_f1(v):
    return (v + 1) // 3


def model_f2(v):
    return (3 - v) & 3


def model(x):
    """the plaintext answer; asserts that nothing leaves its plaintext space on the way"""
    a = [int(sum(int(w) * v for w, v in zip(row, x))) + b for row, b in zip(MODEL_WA, MODEL_BIAS_A)]
    assert all(0 <= v < 1 << BITS_A for v in a), a
    h = [model_f1(v) for v in a]
    b = [int(sum(int(w) * v for w, v in zip(row, h))) for row in MODEL_WB]
    assert all(0 <= v < 1 << BITS_B for v in b), b
    return [model_f2(v) for v in b]


def model_tables(P):
    return (O.trivial_lut_glwe(O.generate_lut(P.N, [model_f1], BITS_A), P), O.trivial_lut_glwe(O.generate_lut(P.N, [model_f2], BITS_B), P))


def model_bias_words():
    return np.array([b << (63 - BITS_A) for b in MODEL_BIAS_A], dtype=np.uint64)


def model_encrypt(ks, run):
    """level-0 encryptions of MODEL_INPUTS[run], messages at 2^(63 - BITS_A)"""
    rng = O.Rng(0xEC50 + run)
    return np.stack([O.encrypt_lwe(rng, ks.lwe_sk, m << (63 - BITS_A), ks.params.lwe_std) for m in MODEL_INPUTS[run]])


def model_decrypt(ks, y):
    return [O.decode(O.decrypt_lwe_raw(row, ks.glwe_sk), BITS_B) for row in y]


# ---- reload: one graph, four runs, other weights of the same shape before the last -------------------------------------------------

def reload_rounds(eng, P, kind=ValueKind.LWE1):
    """a scattered layer (inputs) feeding an in-place one (its results), run three times on new contents, then once more after
    both slots were loaded again: every run gives the words of the weights loaded when it ran.  With SPF_GRAPH_CAPTURE=1 the
    second run captures and the third replays, so the reload falls after the capture."""
    W, K, M1, M2 = words(P, kind), 5, 9, 2
    x = LC.uniform_inputs(0xEC60, 1, K, W)[0]
    wa, ba = weights(0xEC61, M1, K, True)
    wb, bb = weights(0xEC62, M2, M1, False)
    eng.load_lwe_linear_weights(4, wa, ba)
    eng.load_lwe_linear_weights(5, wb, bb)
    g = spf_amd.FheCircuit(eng)
    xs = [g.add_input(kind, row) for row in x]
    a = g.add_lwe_linear(4, xs)
    b = g.add_lwe_linear(5, a)
    out_a, out_b = [g.add_output(n, kind) for n in a], [g.add_output(n, kind) for n in b]
    for rnd in range(4):
        if rnd:
            x[...] = LC.uniform_inputs(0xEC60 + rnd, 1, K, W)[0]      # the same buffers, new contents
        if rnd == 3:
            wa, ba = weights(0xEC63, M1, K, True)
            wb, bb = weights(0xEC64, M2, M1, True)                    # (the second slot gains a bias)
            eng.load_lwe_linear_weights(4, wa, ba)
            eng.load_lwe_linear_weights(5, wb, bb)
        g.run()
        want_a = LC.linear_ref(x, wa, ba)
        assert same_words(np.stack(out_a), want_a), rnd
        assert same_words(np.stack(out_b), LC.linear_ref(want_a, wb, bb)), rnd
    g.close()


# ---- levels of a recording, the way the executor assigns them before it moves anything ---------------------------------------------

def levels(rec) -> list:
    lv = []
    for op, ins in zip(rec.op, rec.inputs):
        lv.append(0 if op < 0 else 1 + max(lv[i] for i in ins))
    return lv
