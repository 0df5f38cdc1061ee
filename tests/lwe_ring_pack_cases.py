"""Leaves, the embedding and the oracle-level reference of ring packing (spf_lwe_ring_pack_*; include/spf_hip.h, "ring packing"),
shared by tests/test_lwe_ring_pack_reference.py (CPU: the composition against the oracle's trace, against plaintext polynomials and
against decryption) and tests/test_gpu_lwe_ring_pack.py (the HIP kernels against the composition, word for word).  Test
infrastructure.

The operation is no function of the reference but a fixed composition of functions the oracle states:
  polynomial_shr_round   R.shr_round           mul_xn   O.glwe_mul_xn          add / sub   wrapping u64
  one automorphism round (polynomial_pow_k, then keyswitch_glwe_to_glwe under ak[round - 1])   glwe_keyswitch_cases.oracle_round
Keys and shapes are those of tests/glwe_keyswitch_cases.py.  The leaves of a case are honest encryptions of messages that are all
different, so that a wrong leaf or node index shows in any output."""
import functools

import numpy as np

import oracle as O
from tests import glwe_keyswitch_cases as KC
from tests import poly_ref as R
from tests import polyref_cases as C

U = np.uint64
LWE1, GLWE1 = 1, 2                     # spf_value_kind
PLAIN_BITS = KC.PLAIN_BITS
SHAPES = KC.SHAPES
LEAVES = {"default128_6x7": 32, "N256k3_7x5": 256, "N16": 80}   # the leaves a case holds, of each kind


def leaf_words(P, kind: int) -> int:
    return P.k * P.N + 1 if kind == LWE1 else (P.k + 1) * P.N


def message(j: int) -> int:
    """message j of a case at PLAIN_BITS bits: all different below 2^12, none 0"""
    return (37 * j + 11) % (1 << PLAIN_BITS)


def embed(P, lwe) -> np.ndarray:
    """the GLWE (k+1, N) whose sample_extract at index 0 is `lwe` and whose body coefficients 1 .. N-1 are 0:
    a_i[0] = lwe[N i], a_i[c] = -lwe[N i + N - c], b[0] = lwe[k N]"""
    lwe = np.asarray(lwe, dtype=U)
    g = np.zeros((P.k + 1, P.N), dtype=U)
    for i in range(P.k):
        a = lwe[P.N * i:P.N * (i + 1)]
        g[i, 0] = a[0]
        g[i, 1:] = U(0) - a[:0:-1]
    g[P.k, 0] = lwe[P.k * P.N]
    return g


def leaf_glwe(P, leaf, kind: int) -> np.ndarray:
    """c^(0) of a leaf: the embedding first, the shift second"""
    g = embed(P, leaf) if kind == LWE1 else np.asarray(leaf, dtype=U).reshape(P.k + 1, P.N)
    return R.shr_round(g, KC.log2n(P))


@functools.lru_cache(maxsize=None)
def leaves(shape: str, kind: int) -> np.ndarray:
    """LEAVES[shape] honest leaves under the case's GLWE key (LWE1: under its flattened form), leaf j an encryption of
    message(j) << (64 - PLAIN_BITS); a GLWE leaf carries it in coefficient 0 and uniform words in every other coefficient
    (the packing must remove them): (count, leaf words)"""
    c = KC.case(shape)
    P, n = c.P, LEAVES[shape]
    rng = np.random.default_rng([0xD0, P.N, P.k, kind])
    enc = [message(j) << (64 - PLAIN_BITS) for j in range(n)]
    if kind == LWE1:
        # the flattened key of sample_extract: LWE coefficient N i + j meets s_i[j]
        out = np.stack([R.lwe_encrypt(rng, c.hk.glwe_sk, m, C.NOISE) for m in enc])
    else:
        msgs = rng.integers(0, 1 << 64, (n, P.N), dtype=U)
        msgs[:, 0] = np.array(enc, dtype=U)
        out = R.glwe_encrypt(rng, c.hk.glwe_sk, msgs, C.NOISE).reshape(n, -1)
    out.setflags(write=False)
    return out


def oracle_ring_pack(c: KC.KsCase, lv, p: int, kind: int) -> np.ndarray:
    """the composition on the p leaves of ONE output, (p, leaf words) -> (k+1, N)"""
    P = c.P
    L, m = KC.log2n(P), p.bit_length() - 1
    assert p == 1 << m and 1 <= p <= P.N and len(lv) == p
    cur = [leaf_glwe(P, leaf, kind) for leaf in lv]
    for lvl in range(1, m + 1):
        cnt = p >> lvl
        nxt = []
        for r in range(cnt):
            E = cur[r]
            Od = O.glwe_mul_xn(cur[r + cnt].reshape(-1), P.N >> lvl, P.N, P.k).reshape(P.k + 1, P.N)
            nxt.append((E + Od) + KC.oracle_round(c, E - Od, L - lvl + 1))
        cur = nxt
    x = cur[0]
    for rnd in range(1, L - m + 1):
        x = x + KC.oracle_round(c, x, rnd)
    return x


@functools.lru_cache(maxsize=None)
def oracle_outputs(shape: str, B: int, p: int, kind: int) -> np.ndarray:
    """the composition on the first B * p leaves of the case, output b from leaves b p .. b p + p - 1: (B, k+1, N), computed
    once in a process"""
    c = KC.case(shape)
    lv = leaves(shape, kind)
    out = np.stack([oracle_ring_pack(c, lv[b * p:(b + 1) * p], p, kind) for b in range(B)])
    out.setflags(write=False)
    return out


def launches(P, p: int) -> int:
    """launches of one slice: a tree level each, the tail unless p = N; p = 1: the leaf's conversion and the trace"""
    return 2 if p == 1 else (p.bit_length() - 1) + (0 if p == P.N else 1)


def check_decrypts(c: KC.KsCase, packed, first_leaf: int, p: int, who: str) -> float:
    """coefficient j N / p of the phase decodes to message(first_leaf + j) and every other coefficient to 0, at PLAIN_BITS bits;
    returns the largest phase error, of the torus"""
    P = c.P
    phase = R.glwe_phase(np.asarray(packed, dtype=U).reshape(P.k + 1, P.N), c.hk.glwe_sk)
    want = np.zeros(P.N, dtype=U)
    want[np.arange(p) * (P.N // p)] = [message(first_leaf + j) for j in range(p)]
    err = float(R.torus_distance(phase, want << U(64 - PLAIN_BITS)).max())
    got = KC.decode(phase)
    assert np.array_equal(got, want), (c.name, who, p, np.argwhere(got != want)[:8].ravel(), err)
    assert err < KC.DECODE_RADIUS, (c.name, who, p, err)
    return err
