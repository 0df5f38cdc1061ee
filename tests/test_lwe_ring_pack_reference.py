"""Ring packing on the oracle alone (tests/lwe_ring_pack_cases.py), no GPU: the embedding against `sample_extract`; the index and
round mapping of the composition on plaintext polynomials; p = 1 against the oracle's `trace`; and decryption of the composition's
outputs at 12 plaintext bits, inside the reference's decode radius (glwe_keyswitch_cases.DECODE_RADIUS — the reference's decode,
not a figure of the code under test).  Measured here on the oracle alone, largest phase error of the torus: N16 1.96e-8 (p = 16,
over all p and both leaf kinds), N256k3_7x5 7.50e-8 (p = 256), default128_6x7 3.27e-8 (p = 32); the radius is 1.22e-4.  (The
leaves' own 2^14 of noise is 8.9e-16; what shows is N/2 units of the shift's rounding and the keyswitch rounds on top.)"""
import numpy as np
import pytest

import oracle as O
from tests import glwe_keyswitch_cases as KC
from tests import lwe_ring_pack_cases as RC
from tests import poly_ref as R

U = np.uint64


@pytest.mark.parametrize("shape", list(RC.SHAPES))
def test_sample_extract_at_0_of_the_embedding_is_the_leaf(shape):
    P = KC.case(shape).P
    for lwe in RC.leaves(shape, RC.LWE1)[:3]:
        g = RC.embed(P, lwe)
        assert np.array_equal(O.sample_extract(g.reshape(-1), 0, P.N, P.k), lwe)
        assert np.array_equal(R.sample_extract(g, 0), lwe)
        assert not g[P.k, 1:].any()


def plain_ring_pack(polys, N: int) -> np.ndarray:
    """the composition on phases: sigma_t acts on a plaintext polynomial as on a ciphertext and the keyswitch keeps the phase"""
    p = len(polys)
    L, m = N.bit_length() - 1, p.bit_length() - 1
    cur = [np.asarray(q, dtype=U) for q in polys]
    for lvl in range(1, m + 1):
        cnt = p >> lvl
        t = (N >> (L - lvl + 1 - 1)) + 1                  # round L - lvl + 1: t = N / 2^(round - 1) + 1 = 2^lvl + 1
        assert t == (1 << lvl) + 1
        nxt = []
        for r in range(cnt):
            E, Od = cur[r], R.mul_monomial(cur[r + cnt], N >> lvl)
            nxt.append((E + Od) + R.automorphism(E - Od, t))
        cur = nxt
    x = cur[0]
    for rnd in range(1, L - m + 1):
        x = x + R.automorphism(x, (N >> (rnd - 1)) + 1)
    return x


@pytest.mark.parametrize("N", [16, 64])
def test_the_plaintext_identity_for_every_p(N):
    """coefficient j N / p of the result is N times coefficient 0 of polynomial j, every other coefficient is 0"""
    rng = np.random.default_rng([0xD1, N])
    p = 1
    while p <= N:
        polys = rng.integers(0, 1 << 64, (p, N), dtype=U)
        got = plain_ring_pack(polys, N)
        want = np.zeros(N, dtype=U)
        want[np.arange(p) * (N // p)] = polys[:, 0] * U(N)
        assert np.array_equal(got, want), (N, p)
        p *= 2


@pytest.mark.parametrize("shape", list(RC.SHAPES))
@pytest.mark.parametrize("kind", [RC.LWE1, RC.GLWE1])
def test_p_1_is_the_trace_of_the_shifted_leaf(shape, kind):
    c = KC.case(shape)
    leaf = RC.leaves(shape, kind)[1]
    want = O.trace(RC.leaf_glwe(c.P, leaf, kind).reshape(-1), c.ak_fft.reshape(-1), c.P).reshape(c.P.k + 1, c.P.N)
    assert np.array_equal(RC.oracle_ring_pack(c, [leaf], 1, kind), want)


DECRYPT = ([("N16", p, k) for p in (1, 2, 4, 8, 16) for k in (RC.LWE1, RC.GLWE1)] +
           [("N256k3_7x5", p, RC.LWE1) for p in (1, 2, 32, 256)] + [("default128_6x7", p, RC.LWE1) for p in (1, 8, 32)])


@pytest.mark.parametrize("shape,p,kind", DECRYPT)
def test_the_composition_decrypts_to_the_messages_at_their_strided_places(shape, p, kind):
    c = KC.case(shape)
    out = RC.oracle_outputs(shape, 1, p, kind)[0]
    err = RC.check_decrypts(c, out, 0, p, "oracle")
    print(f"ring pack {shape:16s} p {p:4d} kind {kind} phase error max {err:.3e} of the torus (decode radius {KC.DECODE_RADIUS:.3e})")


def test_outputs_take_their_own_leaves():
    """output b of a batch packs leaves b p .. b p + p - 1"""
    c = KC.case("N16")
    outs = RC.oracle_outputs("N16", 3, 4, RC.LWE1)
    for b in range(3):
        RC.check_decrypts(c, outs[b], 4 * b, 4, f"output {b}")
