"""The oracle's `keyswitch_glwe_to_glwe`, `polynomial_pow_k` and `trace` against each other and against decryption, without a GPU:
what tests/test_gpu_glwe_keyswitch.py compares the kernels with means what it should (tests/glwe_keyswitch_cases.py)."""
import numpy as np
import pytest

from tests import glwe_keyswitch_cases as KC
from tests import poly_ref as R
from tests import polyref_cases as C

SHAPES = list(KC.SHAPES)


@pytest.mark.parametrize("shape", SHAPES)
def test_folding_the_rounds_is_the_trace_word_for_word(shape):
    c = KC.case(shape)
    want = KC.oracle_traces(shape)
    for i in (0, KC.ITEMS - 1):
        got = KC.oracle_fold(c, c.x[i])
        assert np.array_equal(got, want[i]), (shape, i, np.argwhere(got != want[i])[:8])


@pytest.mark.parametrize("shape", SHAPES)
def test_the_round_is_pow_k_then_the_keyswitch_of_the_exact_reference(shape):
    """the oracle's round against tests/poly_ref.py's exact integers: a wrong exponent, sign or key slice moves the words by a
    uniform amount, the oracle's own floating-point error stays within the model of its transform"""
    c = KC.case(shape)
    P = c.P
    for rnd in (1, KC.log2n(P)):
        t = KC.exponents(P)[rnd - 1]
        assert np.array_equal(KC.oracle_pow_k(P, c.x[1], t), R.automorphism(c.x[1], t)), (shape, rnd)
        exact = R.keyswitch_glwe(R.automorphism(c.x[1], t), c.hk.ak[rnd - 1], P.tr_radix_log, P.tr_count)
        d = float(R.torus_distance(KC.oracle_round(c, c.x[1], rnd), exact).max())
        # tests/polyref_cases.py's model of the transform's rounding, k * count digit x key products, and its cap on a maximum
        bound = 2.0 ** 5.5 * C.sigma_model(P.tr_radix_log, P.k * P.tr_count, P.N)
        print(f"round {rnd:2d} {shape:16s} oracle against exact integers: max {d:.3e}, bound {bound:.3e}")
        assert d <= bound, (shape, rnd, d, bound)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_keyswitch_a_to_b_keeps_the_phase(shape):
    c = KC.case(shape)
    KC.check_switched_phase(c, c.x, KC.oracle_keyswitch(c.P, c.x, c.ksk_fft), "oracle")


def test_the_keyswitch_at_another_radix_keeps_the_phase():
    c = KC.case("default128_6x7")
    _, fft = KC.other_radix_key(c)
    KC.check_switched_phase(c, c.x[:2], KC.oracle_keyswitch(c.P, c.x[:2], fft, KC.OTHER_RADIX), "oracle4x8")


@pytest.mark.parametrize("shape", SHAPES)
def test_can_trace(shape):
    import oracle as O
    c = KC.case(shape)
    ones = KC.all_ones_glwe(c)
    assert np.array_equal(KC.decode(R.glwe_phase(ones, c.hk.glwe_sk)), np.ones(c.P.N, dtype=np.uint64))
    KC.check_can_trace(c, O.trace(ones.reshape(-1), c.ak_fft.reshape(-1), c.P), "oracle")
