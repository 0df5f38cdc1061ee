"""CPU side of the conversion-regime tests: (1) the engineered inputs of tests/conversion_cases.py really reach the regime
their class is named after, witnessed by the doubles the oracle hands to its own f64 -> torus conversion (the kernels are
bit-equal to the oracle through the transform, so the same doubles reach theirs); (2) that conversion against a big-integer
model of the reference's sequence on a dense grid.  The conditions below are conditions on the INPUTS, met with the oracle
alone; tests/test_gpu_conversion_regimes.py then holds the kernels to the oracle's words on the same inputs."""
import collections
import math
from fractions import Fraction

import numpy as np

import oracle as O
from tests import conversion_cases as C
from tests import poly_ref as R
from tests.decomp_ref import M64

P = C.P
Q63 = 1 << 63


def check_class(cls, k, who):
    """k = classify(values of the output polynomial the constant sits in)"""
    band, expo, neg, quirk, sup = k["band"], k["expo"], k["neg"], k["quirk"], k["superset"]
    n = band.size
    count = collections.Counter(band.tolist())
    name = cls.name.split("(")[0]
    if name == "zero":
        assert count == {"zero": n}, (who, count)
    elif name == "sub52":
        assert count == {"sub52": n}, (who, count)
    elif name == "below_52":
        assert count == {"sub52": n} and (expo == 1074).all() and neg.all(), (who, count)
    elif name == "above_52":
        assert count == {"mid": n} and (expo == 1075).all() and neg.all(), (who, count)
    elif name == "mid":
        assert count == {"mid": n} and (expo < 1086).all(), (who, count)
    elif name == "minus_2_63":
        assert count == {"mid": n} and neg.all() and (expo >= 1085).all(), (who, count)
        assert quirk.sum() > 0, (who, "test vector no longer hits the quirk")
    elif name == "plus_2_63":
        assert count == {"mid": n} and not neg.any() and (expo >= 1085).all() and not quirk.any(), (who, count)
        assert sum(1 for x in k["ints"] if x == Q63) > 0, (who, "no value is +2^63 exactly")
    elif name == "below_64":
        assert (expo == 1086).all() and neg.all() and not quirk.any(), (who, sorted(set(expo.tolist())))
    elif name == "in_window":
        assert count == {"window": n} and not sup.any() and not quirk.any(), (who, count, int(sup.sum()))
    elif name == "quirk_in_window":
        assert count == {"window": n} and neg.all(), (who, count)
        assert quirk.sum() > 0, (who, "test vector no longer hits the quirk")
    elif name == "quirk_lookalike":
        assert count == {"window": n} and not neg.any() and not quirk.any(), (who, count)
        assert sup.sum() > 0, (who, "no value makes the superset detector fire")
    elif name == "above_window":
        assert count == {"above": n} and (expo == 1139).all(), (who, count)
    elif name == "mixed":
        win = band == "window"
        regimes = {"zero or below 2^52": np.isin(band, ("zero", "sub52")), "-2^63 (quirk below the window)": quirk & ~win,
                   "+2^63": np.array([x == Q63 for x in k["ints"]]), "window, nothing fires": win & ~sup,
                   "window, quirk": win & quirk, "window, superset only": win & sup & ~quirk}
        empty = [r for r, m in regimes.items() if not m.any()]
        assert not empty, (who, empty)
    elif name == "one_outlier":
        out = np.nonzero(band != "window")[0]
        assert out.size == 1 and not sup.any() and not quirk.any(), (who, out)
        return int(out[0])
    elif name == "one_below_52":
        out = np.nonzero(band != "mid")[0]
        assert out.size == 1 and band[out[0]] == "sub52" and (expo[band == "mid"] == 1075).all(), (who, out)
        return int(out[0])
    else:
        raise AssertionError(f"class {cls.name} has no condition")
    return -1


def test_class_list_and_placements():
    names = {c.name.split("(")[0] for c in C.CMUX_CLASSES}
    assert names >= {"zero", "sub52", "mid", "minus_2_63", "plus_2_63", "below_64", "in_window", "quirk_in_window",
                     "quirk_lookalike", "mixed", "one_outlier"}
    assert {c.outlier for c in C.CMUX_CLASSES if c.name.startswith("one_outlier")} >= {0, 1, 15, 16, 63, 64, 1023, 1024, 2047}
    assert len([c for c in C.CMUX_CLASSES if c.name.startswith("one_outlier")]) >= 17
    assert {c.at for c in C.cmux_cases() if c.cls.name == "mixed"} == set(C.PLACEMENTS) and len(C.PLACEMENTS) == 8
    for cls_list, half in ((C.CMUX_CLASSES, 8), (C.TRACE_CLASSES, 64), (C.PBS_CLASSES, 1 << 15)):
        assert C.by_name(cls_list, "minus_2_63").c * -half == -Q63 and set(C.by_name(cls_list, "minus_2_63").digits) == {-half}


def test_cmux_inputs_reach_their_regime():
    tally = collections.Counter()
    for c in C.cmux_cases():
        r0, lvl0, p0 = c.at
        seen = O.cmux_conversion_input(c.d0.reshape(-1), c.d1.reshape(-1), c.ggsw, P.N, P.k, P.cbs_radix_log, P.cbs_count)
        assert not seen[1 - p0].any(), c.name                     # the other output polynomial: products with zero
        k = C.classify(seen[p0])
        at = check_class(c.cls, k, c.name)
        assert at == c.cls.outlier, (c.name, at)
        # the oracle's conversion of exactly these values, against the big-integer model
        out = O.cmux(c.d0.reshape(-1), c.d1.reshape(-1), c.ggsw, P.N, P.k, P.cbs_radix_log, P.cbs_count).reshape(2, P.N)
        words = out[p0] - c.d0[p0]
        assert np.array_equal(words, C.rust_conversion(k["ints"])), c.name
        if c.cls.name in ("minus_2_63", "quirk_in_window"):
            exact = R.external_product(c.diff(), c.ggsw_rows, P.cbs_radix_log, P.cbs_count)[p0]
            hit = (words == np.uint64(Q63 - 1)) & (exact == np.uint64(Q63))
            assert hit.sum() > 0, (c.name, "test vector no longer hits the quirk")
            assert hit.sum() == k["quirk"].sum(), c.name
        tally[c.cls.name.split("(")[0]] += 1
        if c.at == C.PLACEMENTS[0] or c.cls.outlier >= 0:
            print(f"cmux  {c.name:44s} {dict(collections.Counter(k['band'].tolist()))} quirk {int(k['quirk'].sum())} "
                  f"superset {int(k['superset'].sum())}")
    assert tally["one_outlier"] == len(C.OUTLIER_POSITIONS) and tally["mixed"] == 8


def test_trace_inputs_reach_their_regime():
    """GLEV level 0 sees the mask as built; the levels above see it rotated by one coefficient each (wrapped ones negated),
    which moves the outlier and keeps every whole-polynomial class: all four units of a ciphertext are witnessed"""
    assert C.TRACE_ROUNDS == (0, 10) and C.TRACE_LEVELS == (2, 5)
    for c in C.trace_cases():
        lvl0, p0 = c.at
        for lvl in range(P.cbs_count):
            seen = O.trace_round_conversion_input(c.glwe.reshape(-1), c.ak, lvl, c.rnd)
            assert not seen[1 - p0].any(), c.name
            k = C.classify(seen[p0])
            at = check_class(c.cls, k, f"{c.name} unit {lvl}")
            if lvl == 0:
                assert at == c.cls.outlier, (c.name, at)
                print(f"trace {c.name:44s} {dict(collections.Counter(k['band'].tolist()))} quirk {int(k['quirk'].sum())} "
                      f"superset {int(k['superset'].sum())}")
            if c.cls.name in ("minus_2_63", "quirk_in_window"):
                # the round's key product in exact integer arithmetic: the mask this unit's trace starts from (every earlier
                # round multiplies by zero and leaves it), through the round's automorphism, keyswitched with a zero body
                x = R.shr_round(R.mul_monomial(c.glwe, -lvl), C.LOG_N)
                x[P.k] = 0
                exact = np.uint64(0) - R.keyswitch_glwe(R.automorphism(x, R.trace_exponents(P.N)[c.rnd]), c.ak_rows[c.rnd],
                                                        P.tr_radix_log, P.tr_count)[p0]
                words = np.array([O.f64_to_torus(float(v)) for v in seen[p0]], dtype=np.uint64)
                hit = (words == np.uint64(Q63 - 1)) & (exact == np.uint64(Q63))
                assert hit.sum() > 0, (c.name, lvl, "test vector no longer hits the quirk")
                assert hit.sum() == k["quirk"].sum(), (c.name, lvl)
        for other in (r for r in (0, 5, 10) if r != c.rnd):       # the other rounds multiply by zero: first, middle, last
            assert not O.trace_round_conversion_input(c.glwe.reshape(-1), c.ak, 0, other).any(), (c.name, other)


def test_blind_rotation_inputs_reach_their_regime():
    for name in C.PBS_EDGE_CLASSES:
        cls = C.by_name(C.PBS_CLASSES, name)
        lwe, lut = C.pbs_vector(cls)
        bsk, _ = C.const_key((1, 2, 2, 2), (0, 1, 0, 1), cls.c)          # `_const_key_engine`'s key
        acc = lut.reshape(2, P.N)
        rot = R.mul_monomial(acc, P.N)                                    # a~ = N
        seen = O.cmux_conversion_input(acc.reshape(-1), rot.reshape(-1), bsk, P.N, P.k, P.pbs_radix_log, P.pbs_count)
        assert check_class(cls, C.classify(seen[1]), name) == cls.outlier
        exp = O.generalized_pbs(lwe, lut, bsk, P.replace(lwe_n=1))
        assert np.array_equal(exp.reshape(2, P.N)[1] - acc[1], C.rust_conversion(C.classify(seen[1])["ints"]))


# ----------------------------------------------------------------------------------------------- the conversion itself


def model(x: float) -> int:
    """round half away from zero, v mod 2^64 with the dividend's sign, centre, saturating `as i64` - on exact rationals and
    Python integers (simd/scalar.rs:26-35, 75-119, math/torus.rs:177-192)"""
    a = abs(Fraction(x))
    r = math.floor(a + Fraction(1, 2))
    return int(C.rust_conversion([-r if x < 0 else r])[0])


def oracle_round_and_convert(re: float, im: float):
    """(re, im) through the oracle's own round() and conversion: a flat spectrum is the transform of the polynomial
    re + im X^(N/2), and its inverse is exact (sums of equal values, differences that are zero, a power-of-two scale), so
    `spfo_twisted_fft_reverse` rounds exactly re and im and `spfo_poly_ifft` converts the results"""
    words = O.poly_ifft(np.full(P.N // 2, complex(re, im)))
    rest = np.delete(words, [0, P.N // 2])
    assert not rest.any(), (re, im)
    return int(words[0]), int(words[P.N // 2])


def grid():
    rng = np.random.default_rng(0x6D0D)
    vals = []
    for e in range(0, 121):
        mants = [0, (1 << 52) - 1, 1] + [int(m) for m in rng.integers(0, 1 << 52, 4, dtype=np.uint64)]
        for m in mants:
            x = float(np.array([(e + 1023) << 52 | m], dtype=np.uint64).view(np.float64)[0])
            vals += [x, -x]
    for k in [0, 1, 2, 3, 7, 8, (1 << 31) - 1, 1 << 31, (1 << 51) - 1, 1 << 51, (1 << 52) - 1] + \
             [int(v) for v in rng.integers(0, 1 << 52, 16, dtype=np.uint64)]:
        vals += [k + 0.5, -(k + 0.5)]                                   # ties below 2^52
    for odd in range(1, 128, 2):                                        # +-2^63 * odd up to 2^70
        vals += [float(odd * Q63), -float(odd * Q63)]
    vals += [0.0, -0.0, 0.49999999999999994, -0.49999999999999994, 2.0 ** 116, -2.0 ** 116, float(3 << 115), -float(3 << 115)]
    return vals


def test_f64_to_torus_against_a_big_integer_model_on_a_dense_grid():
    """Every value reaches the oracle's conversion through the oracle's own rounding (`oracle_round_and_convert`), the
    integer-valued ones through `f64_to_torus` directly as well; `model` rounds and converts on exact rationals."""
    vals = grid()
    assert len(vals) > 1800 and len(vals) % 2 == 0
    quirks = ties = 0
    for x, y in zip(vals[0::2], vals[1::2]):
        for v, got in zip((x, y), oracle_round_and_convert(x, y)):
            want = model(v)
            assert got == want, (v.hex(), hex(got), hex(want))
            if v == math.floor(v):
                assert O.f64_to_torus(v) == want, v.hex()
            plain = int(R.float_to_torus(np.array([v]))[0])             # rint (ties to even), mod 2^64, no saturation
            tie = abs(v) < 2.0 ** 52 and abs(v) % 1.0 == 0.5
            r = math.floor(abs(Fraction(v)) + Fraction(1, 2)) * (-1 if v < 0 else 1)
            if r < 0 and r % (1 << 64) == Q63:
                quirks += 1
                assert got == Q63 - 1 and plain == Q63, v.hex()
            elif tie:
                ties += 1
                assert (got - plain) & M64 in (0, 1, M64), v.hex()      # half away from zero against half to even
            else:
                assert got == plain, (v.hex(), hex(got), hex(plain))
    assert quirks >= 64 and ties >= 50
