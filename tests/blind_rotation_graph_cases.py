"""Shared pieces of the tests of blind rotation by an encrypted shift in gate graphs and by handle
(`spf_graph_add_blind_rotation`, `spf_pool_submit_blind_rotation_v`): the graphs both ways, the oracle's x >> s path, and the
one comparison every test uses.  No tolerance anywhere: words are compared."""
import numpy as np

import oracle as O
import spf_amd
from spf_amd import FheOp, ValueKind
from tests.test_gpu_blind_rotation import oracle_loop  # noqa: F401  (the oracle's glwe_mul_xn + cmux loop, re-exported)
from tests.util import to_engine_params

FOUR_WAVE_SCATTERED = "cmux4_kernel<4,4,rot,scattered>"
PER_WG_SCATTERED = "cmux_kernel<4,4,2,rot,scattered>"
GENERIC_ROT = "generic_cmux_rot_kernel"

# test_gpu_generic.py's SMALL16 and TEST1 with the trace and scheme-switch radices its circuit-bootstrap test gives them
SMALL16 = O.DEFAULT_128.replace(lwe_n=5, lwe_std=0.0, N=16, k=1, glwe_std=0.0, pbs_radix_log=6, pbs_count=2, cbs_radix_log=5,
                                cbs_count=3, ks_radix_log=2, ks_count=6, tr_radix_log=6, tr_count=5, ss_radix_log=5, ss_count=6)
TEST1 = O.DEFAULT_128.replace(lwe_n=6, lwe_std=1e-16, N=128, k=2, glwe_std=1e-16, pbs_radix_log=4, pbs_count=3, cbs_radix_log=4,
                              cbs_count=3, ks_radix_log=4, ks_count=3, tr_radix_log=7, tr_count=6, ss_radix_log=3, ss_count=15)


def same_words(got, want) -> bool:
    """THE comparison: the same shape and every 64-bit word equal"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(got.view(np.uint64), want.view(np.uint64)))


def engine_params(P):
    return to_engine_params(P).replace(tr_radix_log=P.tr_radix_log, tr_radix_count=P.tr_count,
                                       ss_radix_log=P.ss_radix_log, ss_radix_count=P.ss_count)


def random_selectors(seed, n, P):
    """random complex values at 2^58 (test_gpu_blind_rotation.py's _shift): n selectors"""
    out = np.empty((n, P.cbs_ggsw_fft_len), dtype=np.complex128)
    v = out.view(np.float64)
    v[...] = np.random.default_rng(seed).standard_normal(v.shape)
    v *= 2.0 ** 58
    return out


def rotation_graph(eng, glwes, sels, log_stride, composed=False, circuit=None):
    """one GGSW input per bit shared by all items, one GLWE input per item, every rotated item an output.  composed: the same
    words from MulXN(2N - r) + CMux nodes.  -> (graph, [output arrays])"""
    N = eng.params.polynomial_degree
    g = circuit if circuit is not None else spf_amd.FheCircuit(eng)
    s = [g.add_input(ValueKind.GGSW1, v) for v in sels]
    outs = []
    for x in glwes:
        acc = g.add_input(ValueKind.GLWE1, x)
        if composed:
            for i, sel in enumerate(s):
                high = g.add_op(FheOp.MulXN, [acc], 2 * N - (1 << (i + log_stride)))
                acc = g.add_op(FheOp.CMux, [sel, acc, high])
        else:
            acc = g.add_blind_rotation(acc, s, log_stride)
        outs.append(g.add_output(acc, ValueKind.GLWE1))
    return g, outs


def packed_glwe(rng, sk, P, value, n_bits):
    """bit j of `value` at coefficient j, one plaintext bit (spf_amd.packed_plaintext << 63)"""
    pt = np.zeros(P.N, dtype=np.uint64)
    for j in range(n_bits):
        pt[j] = ((value >> j) & 1) << 63
    return O.encrypt_glwe(rng, sk, pt, P.N, P.k, P.glwe_std)


def oracle_shift_right(P, ks, ak, ssk, x_ct, s_ct, s_bits, x_bits):
    """x >> s with both packed: unpack s, KeyswitchL1toL0 and CircuitBootstrap per bit, the rotation by the bits, unpack.
    -> (the rotated GLWE, its x_bits LWEs)"""
    acc = x_ct
    for i in range(s_bits):
        l0 = O.keyswitch_lwe(O.sample_extract(s_ct, i, P.N, P.k), ks.ksk, P.k * P.N, P.lwe_n, P.ks_radix_log, P.ks_count)
        sel = O.circuit_bootstrap(l0, ks.bsk_fft, ak, ssk, P)
        acc = O.cmux(acc, O.glwe_mul_xn(acc, 2 * P.N - (1 << i), P.N, P.k), sel, P.N, P.k, P.cbs_radix_log, P.cbs_count)
    return acc, [O.sample_extract(acc, j, P.N, P.k) for j in range(x_bits)]


def shift_right_graph(g, x, s, s_bits, x_bits):
    """the same steps as nodes of `g` on the packed GLWE nodes x and s -> (output array of the rotated GLWE, of its LWEs)"""
    sels = [g.add_op(FheOp.CircuitBootstrap, [g.add_op(FheOp.KeyswitchL1toL0, [b])]) for b in g.add_unpack(s, s_bits)]
    rotated = g.add_blind_rotation(x, sels)
    return g.add_output(rotated, ValueKind.GLWE1), [g.add_output(b, ValueKind.LWE1) for b in g.add_unpack(rotated, x_bits)]
