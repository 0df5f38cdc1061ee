"""Shared pieces of the tests of the bootstraps by a caller's table and of the public functional keyswitch in gate graphs and by
handle (`SPF_OP_PBS_UNIVARIATE`, `SPF_OP_PBS_BIVARIATE`, `spf_graph_add_public_functional_keyswitch`): the three contexts with
their keys, the operand pool of a keyswitch node, the mixed chain and the one comparison every test uses.  No tolerance anywhere
but in the decrypt-level case: words are compared, against the batch entry points on the same rows and against the oracle."""
import functools

import numpy as np

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests.blind_rotation_graph_cases import SMALL16, TEST1, engine_params, same_words  # noqa: F401  (re-exported)
from tests.util import keyset, random_glwe, random_lwe_batch

CONTEXTS = ["tuned", "n128k2", "n16k1"]
NO_KEY = 3


def pack(left, right, p: int) -> np.ndarray:
    """left * 2^p + right, wrapping: the input of the univariate bootstrap a bivariate one stands for"""
    return np.asarray(left, dtype=np.uint64) * np.uint64(1 << p) + np.asarray(right, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def keys_of(which):
    """(oracle parameters, key set, automorphism key, scheme-switch key): DEFAULT_128 with a short LWE side (the tuned kernels;
    test_gpu_values.py's keys), and the generic contexts at (N, k) = (128, 2) and (16, 1)"""
    if which == "tuned":
        ks = keyset(0x5EED0001, 12)
        r = O.Rng(0x7A11)
    else:
        ks = O.gen_keyset(0x5EED0009, TEST1 if which == "n128k2" else SMALL16)
        r = O.Rng(0x7A12)
    return ks.params, ks, O.gen_auto_key_fft(r, ks.glwe_sk, ks.params), O.gen_ssk_fft(r, ks.glwe_sk, ks.params)


def load_keys(eng, which):
    _, ks, ak, ssk = keys_of(which)
    eng.load_bootstrap_key(ks.bsk_fft)
    eng.load_keyswitch_key(ks.ksk)
    eng.load_automorphism_key(ak)
    eng.load_scheme_switch_key(ssk)


def make_engine(which):
    e = spf_amd.Engine(engine_params(keys_of(which)[0]))
    load_keys(e, which)
    return e


@functools.lru_cache(maxsize=2)
def pufks_key(N, k, n, count, seed=0):
    """uniform words (n, count, k+1, N): parity does not need an honest key"""
    return np.random.default_rng([0xD0, N, k, n, count, seed]).integers(0, 1 << 64, (n, count, k + 1, N), dtype=np.uint64)


def dimension(P, kind) -> int:
    return P.lwe_n if ValueKind(kind) == ValueKind.LWE0 else P.k * P.N


class RowPool:
    """six LWE nodes of one kind from three levels of `g`, each an output so that the tests know its words.  LWE1: two inputs, two
    bits unpacked from an input, two from a computed GLWE.  LWE0 (the planner pulls a keyswitch up against its first user): two
    inputs, two keyswitch results, and two keyswitch results that depend on a public functional keyswitch of those four — which
    needs the key of the LWE0 dimension loaded"""

    def __init__(self, g, P, kind, seed):
        kind = ValueKind(kind)
        l1 = random_lwe_batch(seed, 4, P.k * P.N)
        glwe = random_glwe(seed + 1, 2, P.glwe_len)
        self.nodes = []
        if kind == ValueKind.LWE0:
            x = random_lwe_batch(seed + 2, 2, P.lwe_n)
            self.nodes += [g.add_input(ValueKind.LWE0, v) for v in x]
            self.nodes += [g.add_op(FheOp.KeyswitchL1toL0, [g.add_input(ValueKind.LWE1, v)]) for v in l1[:2]]
            first = g.add_public_functional_keyswitch(self.nodes)
            self.nodes += [g.add_op(FheOp.KeyswitchL1toL0, [b]) for b in g.add_unpack(first, 2)]
        else:
            self.nodes += [g.add_input(ValueKind.LWE1, v) for v in l1[:2]]
            self.nodes += g.add_unpack(g.add_input(ValueKind.GLWE1, glwe[0]), 2)
            self.nodes += g.add_unpack(g.add_op(FheOp.Not, [g.add_input(ValueKind.GLWE1, glwe[1])]), 2)
        self.outs = [g.add_output(n, kind) for n in self.nodes]

    def pick(self, output: int, count: int):
        """indices into the pool of the `count` rows of output `output`: every level, and repeats from the seventh row on"""
        return [(2 * output + 5 * j) % 6 for j in range(count)]


def mixed_chain(g, glwe, lut, W, p):
    """input GLWE -> add_unpack(W) -> keyswitch -> bivariate table (digit i with digit i + 1) -> public functional keyswitch of the
    W results -> CMUX with a circuit-bootstrapped selector (the first keyswitched digit) against the input -> output.
    -> {name: output array} of every stage"""
    x = g.add_input(ValueKind.GLWE1, glwe)
    t = g.add_input(ValueKind.GLWE1, lut)
    bits = g.add_unpack(x, W)
    l0 = [g.add_op(FheOp.KeyswitchL1toL0, [b]) for b in bits]
    biv = [g.add_op(FheOp.PBS_BIVARIATE, [l0[i], l0[(i + 1) % W], t], p) for i in range(W)]
    packed = g.add_public_functional_keyswitch(biv)
    sel = g.add_op(FheOp.CircuitBootstrap, [l0[0]])
    out = g.add_op(FheOp.CMux, [sel, packed, x])
    return {"l0": [g.add_output(n, ValueKind.LWE0) for n in l0], "biv": [g.add_output(n, ValueKind.LWE1) for n in biv],
            "packed": g.add_output(packed, ValueKind.GLWE1), "sel": g.add_output(sel, ValueKind.GGSW1),
            "out": g.add_output(out, ValueKind.GLWE1)}


def mixed_chain_by_batch_calls(eng, glwe, lut, W, p):
    """the same rows through the batch entry points, a host round trip after every one"""
    l0 = eng.keyswitch_lwe_l1_lwe_l0(eng.glwe_unpack_l1(glwe[None], W)[0])
    biv = eng.pbs_bivariate(l0, np.roll(l0, -1, axis=0), lut, p)
    packed = eng.public_functional_keyswitch(biv[None])[0]
    sel = eng.circuit_bootstrap(l0[:1])[0]
    return {"l0": l0, "biv": biv, "packed": packed, "sel": sel, "out": eng.cmux(sel[None], packed[None], glwe[None])[0]}
