"""A gate graph evaluated by the oracle: `evaluate(rec, P, keys)` walks the nodes of a `spf_amd.RecordedCircuit` in order and
gives the value of every node, in the expressions the hand-made tests already hold the library to (tests/test_gpu_values.py,
test_gpu_graph.py, test_gpu_pbs_graph.py, test_gpu_blind_rotation_graph.py, test_gpu_packed_graph.py).  No engine, no device:
`oracle` and the numpy references of tests/ only.  `planned_levels` restates the level passes of the executor's plan()
(spf_graph.hpp) so that a generator can say on which level a node runs and a failure message can name it."""
from collections import namedtuple

import numpy as np

import oracle as O
from spf_amd import FheOp, TableOp, ValueKind
from spf_amd.graph import (NODE_GLWE_AUTOMORPHISM, NODE_GLWE_KEYSWITCH, NODE_GLWE_POLY_LINEAR, NODE_GLWE_TRACE, NODE_LWE_LINEAR, NODE_PACK,
                           NODE_PUFKS, NODE_ROT_CMUX, NODE_UNPACK)
from tests import glwe_keyswitch_cases as KC
from tests import glwe_poly_cases as GC
from tests import lwe_linear_cases as LC
from tests import pbs_graph_cases as K
from tests import pufks_cases as PC
from tests.polyref_cases import key_fft

# ks: oracle KeySet; ak / ssk: automorphism and scheme-switch keys; pufks: None or (key as loaded (n, count, k+1, N), log, count);
# linear: None or the weight slots as loaded, {slot: (weights int64 (M, K), bias uint64 (M,) or None)};
# glwe_ksk: None or the GLWE keyswitch-key slots as loaded, {slot: (words (k, L, k+1, N), radix_log, radix_count)};
# glwe_poly: None or the polynomial weight slots as loaded, {slot: (CSR triple, bias (M, N) or None, (M, K))}
Keys = namedtuple("Keys", "ks ak ssk pufks linear glwe_ksk glwe_poly", defaults=(None, None, None, None))

_BOOTSTRAPS = (int(FheOp.CircuitBootstrap), int(TableOp.PBS_UNIVARIATE), int(TableOp.PBS_BIVARIATE))


def keys_of(which, pufks=None, linear=None, glwe_ksk=None, glwe_poly=None) -> Keys:
    """the keys of a context of pbs_graph_cases.CONTEXTS, with the public-functional-keyswitch key, the weight slots of the
    linear maps, the GLWE keyswitch-key slots and the polynomial weight slots if they are loaded"""
    _, ks, ak, ssk = K.keys_of(which)
    return Keys(ks, ak, ssk, pufks, linear, glwe_ksk, glwe_poly)


def kind_name(rec, i) -> str:
    op = rec.op[i]
    if op == -1:
        return f"Input{ValueKind(rec.kind[i]).name}"
    if op == -2:
        return f"Trivial{ValueKind(rec.kind[i]).name}({rec.param[i]})"
    names = {NODE_UNPACK: "Unpack", NODE_PACK: "Pack", NODE_ROT_CMUX: "RotCMux", NODE_PUFKS: "PublicFunctionalKeyswitch",
             NODE_LWE_LINEAR: "LweLinear", NODE_GLWE_POLY_LINEAR: "GlwePolyLinear", NODE_GLWE_KEYSWITCH: "GlweKeyswitch",
             NODE_GLWE_AUTOMORPHISM: "GlweAutomorphism", NODE_GLWE_TRACE: "GlweTrace"}
    return names[op] if op in names else (TableOp(op).name if op in TableOp._value2member_map_ else FheOp(op).name)


def trivial(P, kind, bit) -> np.ndarray:
    """spf_graph.hpp's constants: zero mask, bit << 63 in the body (GLEV: bit * q / B^(j+1) in the body of GLWE j)"""
    kind, bit = ValueKind(kind), int(bit) & 1
    if kind == ValueKind.GLEV1:
        v = np.zeros((P.cbs_count, P.glwe_len), dtype=np.uint64)
        for j in range(P.cbs_count):
            v[j, P.k * P.N] = np.uint64(bit << (64 - P.cbs_radix_log * (j + 1)))
        return v.reshape(-1)
    words = {ValueKind.LWE0: P.lwe_n + 1, ValueKind.LWE1: P.k * P.N + 1, ValueKind.GLWE1: P.glwe_len}[kind]
    v = np.zeros(words, dtype=np.uint64)
    v[P.lwe_n if kind == ValueKind.LWE0 else P.k * P.N] = np.uint64(bit << 63)
    return v


_FFT_OF = []    # (key, its transform) of the last two keys: a level-1 key of the tuned set is 268 MB
_KSK_FFT_OF = []    # the same for GLWE keyswitch keys (a few hundred KB each): the last two tables of three slots


def _key_fft_once(key, cache=_FFT_OF, keep=2):
    for k, f in cache:
        if k is key:
            return f
    cache.append((key, key_fft(key)))
    del cache[:-keep]
    return cache[-1][1]


def oracle_round(P, ak_fft, x, rnd: int) -> np.ndarray:
    """glwe_keyswitch_cases.oracle_round for a context that is no KsCase: round `rnd` in 1 .. log2 N of the trace's loop on the GLWE
    x (k+1, N), without the add, under the automorphism key in transformed form as the contexts load it (any shape; row rnd - 1 of
    its log2 N rows is the round's keyswitch key)"""
    rows = np.asarray(ak_fft).reshape(KC.log2n(P), -1)
    return KC.oracle_keyswitch(P, KC.oracle_pow_k(P, np.asarray(x, dtype=np.uint64).reshape(P.k + 1, P.N), KC.exponents(P)[rnd - 1]), rows[rnd - 1])


def evaluate(rec, P, keys: Keys, hosts=None):
    """-> [value of every node]: uint64 words, complex128 for GGSW1.  hosts: {input node: array} instead of rec.host"""
    ks, N, k, h = keys.ks, P.N, P.k, P.N // 2
    cb = (N, k, P.cbs_radix_log, P.cbs_count)
    pufks_fft = _key_fft_once(keys.pufks[0]) if keys.pufks is not None else None
    ggsw_const = {}
    vals = []

    def cmux(sel, a, b):
        return O.cmux(a, b, sel, *cb)

    for i, op in enumerate(rec.op):
        x = [vals[j] for j in rec.inputs[i]]
        par = rec.param[i]
        if op == -1:
            src = rec.host[i] if hosts is None or i not in hosts else hosts[i]
            dt = np.complex128 if rec.kind[i] == int(ValueKind.GGSW1) else np.uint64
            v = np.ascontiguousarray(src).view(dt).reshape(-1).copy()
        elif op == -2 and rec.kind[i] == int(ValueKind.GGSW1):
            if par & 1 not in ggsw_const:   # Evaluation::new: the circuit bootstrap of the trivial level-0 LWE
                ggsw_const[par & 1] = O.circuit_bootstrap(trivial(P, ValueKind.LWE0, par), ks.bsk_fft, keys.ak, keys.ssk, P)
            v = ggsw_const[par & 1]
        elif op == -2:
            v = trivial(P, rec.kind[i], par)
        elif op in (int(FheOp.SampleExtract), NODE_UNPACK):
            v = O.sample_extract(x[0], par, N, k)
        elif op == int(FheOp.KeyswitchL1toL0):
            v = O.keyswitch_lwe(x[0], ks.ksk, k * N, P.lwe_n, P.ks_radix_log, P.ks_count)
        elif op == int(FheOp.Not):
            v = O.glwe_not(x[0], N, k)
        elif op == int(FheOp.GlweAdd):
            v = O.glwe_xor(x[0], x[1], N, k)
        elif op == int(FheOp.MulXN):
            v = O.glwe_mul_xn(x[0], par % (2 * N), N, k)
        elif op == int(FheOp.CMux):
            v = cmux(x[0], x[1], x[2])
        elif op == int(FheOp.GlevCMux):
            a, b = x[1].reshape(P.cbs_count, -1), x[2].reshape(P.cbs_count, -1)
            v = np.concatenate([cmux(x[0], a[j], b[j]) for j in range(P.cbs_count)])
        elif op == int(FheOp.MultiplyGgswGlwe):
            fft = O.glwe_ggsw_mad(np.zeros((k + 1) * h, dtype=np.complex128), x[1], x[0], *cb)
            v = np.concatenate([O.poly_ifft(fft[q * h:(q + 1) * h]) for q in range(k + 1)])
        elif op == int(FheOp.SchemeSwitch):
            v = O.scheme_switch_fft(x[0].reshape(P.cbs_count, -1), keys.ssk, P)
        elif op == int(FheOp.CircuitBootstrap):
            v = O.circuit_bootstrap(x[0], ks.bsk_fft, keys.ak, keys.ssk, P)
        elif op == int(TableOp.PBS_UNIVARIATE):
            v = O.pbs_univariate(x[0], x[1], ks.bsk_fft, P)
        elif op == int(TableOp.PBS_BIVARIATE):
            v = O.pbs_univariate(K.pack(x[0], x[1], par), x[2], ks.bsk_fft, P)
        elif op == NODE_ROT_CMUX:       # (selector, accumulator), rotation par: blind_rotation_graph_cases.oracle_shift_right
            v = O.cmux(x[1], O.glwe_mul_xn(x[1], 2 * N - par, N, k), x[0], *cb)
        elif op == NODE_PACK:
            v = np.zeros(P.glwe_len, dtype=np.uint64)
            for j, g in enumerate(x):
                v = v + O.glwe_mul_xn(g, j, N, k)
        elif op == NODE_PUFKS:
            key, log, count = keys.pufks
            assert key.shape[0] == x[0].size - 1, "the key's dimension is not the operands'"
            v = PC.pufks_oracle(np.stack(x), pufks_fft, N, k, log, count).reshape(-1)
        elif op == NODE_LWE_LINEAR:     # row par of the layer: the M nodes of one call share the operand list and the slot
            slot, rows = rec.linear_of(i)
            w, bias = keys.linear[slot]
            assert np.shape(w) == (rows, len(x)), f"node {i}: slot {slot} holds {np.shape(w)} weights, the layer is {(rows, len(x))}"
            v = LC.linear_ref(np.stack(x), w, bias)[par]
        elif op == NODE_GLWE_POLY_LINEAR:   # row par of the layer, likewise
            slot, rows = rec.linear_of(i)
            triple, bias, shape = keys.glwe_poly[slot]
            assert tuple(shape) == (rows, len(x)), f"node {i}: slot {slot} holds {tuple(shape)} weights, the layer is {(rows, len(x))}"
            v = GC.poly_linear_ref(np.stack(x).reshape(1, len(x), k + 1, N), triple, rows, len(x), bias)[0, par]
        elif op == NODE_GLWE_KEYSWITCH:     # under the key of slot par, at the key's own radix
            words, log, count = keys.glwe_ksk[par]
            v = KC.oracle_keyswitch(P, x[0].reshape(k + 1, N), _key_fft_once(words, _KSK_FFT_OF, 6), (log, count))
        elif op == NODE_GLWE_AUTOMORPHISM:  # round par of the trace's loop: x(X^t) switched back under row par - 1 of the key
            v = oracle_round(P, keys.ak, x[0], par)
        elif op == NODE_GLWE_TRACE:
            v = O.trace(x[0], np.asarray(keys.ak).reshape(-1), P)
        else:
            raise ValueError(f"node {i}: unknown operation {op}")
        vals.append(np.asarray(v).reshape(-1))
    return vals


def planned_levels(rec):
    """the level of every node as the planner chooses it (spf_graph_plan.hpp, assign_levels): as soon as possible; the three bootstrap kinds moved to common
    levels within their slack; SampleExtract and KeyswitchL1toL0 pulled up against their first user.  Inputs and constants: 0"""
    n = len(rec.op)
    level = [0] * n
    for i in range(n):
        if rec.op[i] >= 0:
            level[i] = 1 + max((level[j] for j in rec.inputs[i]), default=0)
    top = max(level, default=0)
    alap = [top] * n
    for i in reversed(range(n)):
        if rec.op[i] >= 0:
            for j in rec.inputs[i]:
                if rec.op[j] >= 0:
                    alap[j] = min(alap[j], alap[i] - 1)
    fixed, done = [0] * n, [False] * n
    for kind in _BOOTSTRAPS:
        ids = sorted((i for i in range(n) if rec.op[i] == kind), key=lambda i: (alap[i], i))
        for lead in ids:
            if not done[lead]:
                for i in ids:
                    if not done[i] and level[i] <= alap[lead]:
                        done[i], fixed[i] = True, alap[lead]
    for i in range(n):
        if rec.op[i] >= 0:
            level[i] = max(1 + max((level[j] for j in rec.inputs[i]), default=0), fixed[i])
    first_user = [None] * n
    for i in reversed(range(n)):
        if rec.op[i] < 0:
            continue
        if rec.op[i] in (int(FheOp.KeyswitchL1toL0), int(FheOp.SampleExtract)) and first_user[i] is not None:
            level[i] = max(level[i], first_user[i] - 1)
        for j in rec.inputs[i]:
            first_user[j] = level[i] if first_user[j] is None else min(first_user[j], level[i])
    return level


def first_difference(rec, got, want, levels=None):
    """None, or the message naming the lowest differing output node: its kind, its level and its operands"""
    levels = planned_levels(rec) if levels is None else levels
    bad = sorted({node for at, node in enumerate(rec.outputs) if not K.same_words(got[at], want[node])})
    if not bad:
        return None
    i = bad[0]
    ops = ", ".join(f"{j}:{kind_name(rec, j)}@{levels[j]}" for j in rec.inputs[i][:8]) + (" ..." if len(rec.inputs[i]) > 8 else "")
    return (f"{len(bad)} output nodes differ, lowest node {i} of {len(rec.op)}: {kind_name(rec, i)} param {rec.param[i]} "
            f"level {levels[i]} operands [{ops}]")
