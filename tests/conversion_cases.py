"""Inputs engineered to land on a chosen side of every window of the kernels' f64 -> torus conversions (test infrastructure;
shared by tests/test_conversion_regimes.py, CPU, and tests/test_gpu_conversion_regimes.py).

The trick is `_const_key_engine`'s (tests/test_gpu_parity.py): a key whose only non-zero polynomial, at one (row, level, poly),
is the constant c (the polynomial c X^0).  The output polynomial `poly` of the external product is then digit_j0(word_i) * c,
coefficient by coefficient, j0 = count - 1 - level (tests/poly_ref.py `_glev_digits`), and the word of each coefficient sets
its digit.  Magnitude, sign and value mod 2^64 of every value the conversion sees are chosen that way; the oracle's own
pre-conversion doubles (oracle `cmux_conversion_input`, `trace_round_conversion_input`) are the witness that they got there.

A class is (digit pattern over the N coefficients, c, log2 of a power-of-two factor applied to the key's spectrum).  With
half = B/2 the most negative digit (8 for the 4 x 4-bit CMUX radix, 64 for the trace's 6 x 7 bits, 2^15 for the bootstrap's
2 x 16), the constants are the CMUX ones scaled by 8 / half, so that -half * c is the same value at every radix.
"""
from dataclasses import dataclass

import numpy as np

import oracle as O
from tests.decomp_ref import M64, digits_array
from tests.polyref_cases import key_fft

P = O.DEFAULT_128
N = P.N

# one coefficient out of the window: the first and last coefficients, the neighbours of the lane, half-wave and half-polynomial
# boundaries (15 | 16, 63 | 64, 1023 | 1024), eight seeded random positions, and one in every block of 128 coefficients (a lane of the hand-written kernels holds 16 values 128 coefficients apart: every slot of the 16 is hit)
OUTLIER_POSITIONS = tuple(dict.fromkeys(
    [0, 1, 15, 16, 63, 64, 1023, 1024, 2047]
    + [int(p) for p in np.random.default_rng(0x0071).integers(0, N, 8)]
    + [128 * j + 37 for j in range(16)]))


@dataclass(frozen=True)
class Cls:
    name: str
    c: int                  # the key constant, a signed 64-bit integer
    digits: tuple           # N digits
    scale_log2: int = 0     # the key's spectrum times 2^scale_log2 (keys arrive in the transform domain)
    outlier: int = -1       # position of the one coefficient outside the class's regime

    @property
    def d(self) -> np.ndarray:
        return np.array(self.digits, dtype=np.int64)


def _rng(*key):
    return np.random.default_rng([0xC0, *key])


def classes(half: int) -> list:
    """the class list at a radix whose digits lie in [-half, half - 1]"""
    assert half >= 8 and half & (half - 1) == 0
    u = (1 << 63) // half                         # -half * u = -2^63
    r = _rng(half)
    full = lambda d: tuple([d] * N)               # noqa: E731
    small = np.arange(-8, 8)
    nonzero = r.choice(small[small != 0], N)
    even = r.choice(np.array([-8, -6, -4, 4, 6]), N)      # |d| = 2 is 2^64 itself: the transform's rounding takes it below
    out = [
        Cls("zero", -(1 << 63), full(0)),
        Cls("sub52", 1 << 10, tuple(nonzero)),
        Cls("below_52", 3 * (u >> 13), full(-half)),                  # -3 * 2^50
        Cls("above_52", 3 * (u >> 12), full(-half)),                  # -3 * 2^51 = -1.5 * 2^52
        Cls("mid", u >> 5, tuple(nonzero * (half // 8))),             # 2^55 <= |v| <= 2^58
        Cls("minus_2_63", u, full(-half)),
        Cls("plus_2_63", -u, full(-half)),
        Cls("below_64", 3 * (u >> 1), full(-half)),                   # -3 * 2^62: exponent 1086
        Cls("in_window", -(1 << 63), tuple(even)),                    # even multiples of 2^63 in [2^65, 2^66]
        Cls("quirk_in_window", 3 * u, full(-half)),                   # -3 * 2^63
        Cls("quirk_lookalike", -3 * u, full(-half)),                  # +3 * 2^63
        Cls("mixed", -(1 << 63), tuple(r.integers(-8, 8, N))),
        Cls("above_window", 3 * (u >> 1), full(-half), scale_log2=53),    # -3 * 2^115 = -1.5 * 2^116: exponent 1139
    ]
    for p in OUTLIER_POSITIONS:
        d = even.copy()
        d[p] = 0
        out.append(Cls(f"one_outlier({p})", -(1 << 63), tuple(d), outlier=p))
    for p in (0, 1023, 1024, 2047, 128 * 5 + 37):
        d = np.full(N, -half)
        d[p] = -half // 2                                             # -0.75 * 2^52 among -1.5 * 2^52
        out.append(Cls(f"one_below_52({p})", 3 * (u >> 12), tuple(d), outlier=p))
    return out


def by_name(cls_list, name: str) -> Cls:
    return next(c for c in cls_list if c.name == name)


def digit_words(d, radix_log: int, count: int, j: int, bits: int = 64) -> np.ndarray:
    """words of `bits` bits whose digit j (least significant first) at radix 2^radix_log x count OF A 64-BIT WORD is d; the
    digits above j are whatever the carries make them, the ones below are zero"""
    shift = 64 - radix_log * count + radix_log * j
    w = [(int(x) << shift) & ((1 << bits) - 1) for x in np.asarray(d).reshape(-1)]
    w = np.array(w, dtype=np.uint64)
    assert np.array_equal(digits_array(w, radix_log, count)[:, j], np.asarray(d).reshape(-1)), "digit not representable"
    assert not digits_array(w, radix_log, count)[:, :j].any()
    return w


def const_key(shape, at, c: int, scale_log2: int = 0) -> np.ndarray:
    """transform-domain key of time-domain shape `shape` + (N,), zero but for the constant c at index `at`"""
    rows = np.zeros(tuple(shape) + (N,), dtype=np.uint64)
    rows[tuple(at) + (0,)] = c & M64
    return key_fft(rows) * 2.0 ** scale_log2, rows


# ----------------------------------------------------------------------------------------------- CMUX family (4 x 4 bits)

CMUX_CLASSES = classes(8)
PLACEMENTS = [(r0, lvl0, p0) for r0 in (0, 1) for lvl0 in (0, P.cbs_count - 1) for p0 in (0, 1)]   # both rows, top and bottom level


@dataclass
class CmuxCase:
    name: str
    cls: Cls
    at: tuple               # (row, level, poly)
    d0: np.ndarray          # (k+1, N)
    d1: np.ndarray
    ggsw: np.ndarray        # transform domain, flat
    ggsw_rows: np.ndarray   # time domain (k+1, L, k+1, N); exact arithmetic is valid when cls.scale_log2 == 0

    def diff(self):
        return self.d1 - self.d0


def cmux_case(cls: Cls, at, radix_log=P.cbs_radix_log, count=P.cbs_count) -> CmuxCase:
    r0, lvl0, p0 = at
    rng = _rng(1, r0, lvl0, p0, sum(map(ord, cls.name)))
    d0 = rng.integers(0, 1 << 64, (P.k + 1, N), dtype=np.uint64)
    diff = rng.integers(0, 1 << 64, (P.k + 1, N), dtype=np.uint64)      # the other row meets zero key polynomials
    diff[r0] = digit_words(cls.d, radix_log, count, count - 1 - lvl0)
    g, rows = const_key((P.k + 1, count, P.k + 1), at, cls.c, cls.scale_log2)
    return CmuxCase(f"{cls.name}@row{r0}-level{lvl0}-poly{p0}", cls, at, d0, d0 + diff, g, rows)


def cmux_cases() -> list:
    """every whole-polynomial class at every placement; the one-outlier classes with the placements cycled through them"""
    out = []
    i = 0
    for cls in CMUX_CLASSES:
        if cls.outlier < 0:
            out += [cmux_case(cls, at) for at in PLACEMENTS]
        else:
            out.append(cmux_case(cls, PLACEMENTS[i % len(PLACEMENTS)]))
            i += 1
    return out


DOOR_CLASSES = ("mixed", "quirk_in_window", "minus_2_63", "quirk_lookalike", "one_outlier(0)", "one_outlier(1023)",
                f"one_outlier({128 * 9 + 37})")


def door_cases() -> list:
    """the classes every other entry point of the CMUX kernels runs, body placement at the top level and mask at the bottom"""
    return [cmux_case(by_name(CMUX_CLASSES, n), PLACEMENTS[(3 * i) % len(PLACEMENTS)]) for i, n in enumerate(DOOR_CLASSES)]


# ----------------------------------------------------------------------------------------------- trace (6 x 7 bits)

TRACE_CLASSES = classes(64)
LOG_N = N.bit_length() - 1
# The words a round decomposes are the mask of shr_round(input, log2 N): 53-bit integers.  Digit j of the 42 top bits of a
# 64-bit word covers bits 22 + 7j .. 28 + 7j, so only the digits j <= 3 can take every value in [-64, 63]: j = 3 (key level 2)
# is the highest level a chosen digit reaches, j = 0 (level 5) the lowest.
TRACE_LEVELS = (P.tr_count - 1 - 3, P.tr_count - 1)
TRACE_ROUNDS = (0, LOG_N - 1)


@dataclass
class TraceCase:
    name: str
    cls: Cls
    rnd: int
    at: tuple               # (level, poly) of the round's keyswitch key (k = 1: one row)
    glwe: np.ndarray        # (k+1, N) input of mod_switch_trace_and_rotate
    ak: np.ndarray          # transform domain, flat
    ak_rows: np.ndarray     # time domain (log2 N, k, L, k+1, N); exact arithmetic is valid when cls.scale_log2 == 0


def trace_case(cls: Cls, rnd: int, at) -> TraceCase:
    """Only round `rnd` has a non-zero key, so the mask every earlier round leaves is the input's.  Round `rnd` decomposes
    mask(X^t), t = N / 2^rnd + 1: coefficient i of the mask lands at i t mod N, negated when floor(i t / N) is odd.  A negated
    word carries the negated digit (-64 stays -64), which every class here admits: the sign-sensitive ones use -64 only, the
    others are sets of digits closed under negation or magnitudes.  GLEV level 0 sees the mask as given (level l sees it
    times X^-l: l wrapped coefficients negated, the others shifted)."""
    lvl0, p0 = at
    rng = _rng(2, rnd, lvl0, p0, sum(map(ord, cls.name)))
    t = N // (1 << rnd) + 1
    want = cls.d                                                     # digit wanted at each coefficient of mask(X^t)
    src = (np.arange(N) * t) % N
    x = digit_words(want[src], P.tr_radix_log, P.tr_count, P.tr_count - 1 - lvl0, bits=53)
    glwe = rng.integers(0, 1 << 64, (P.k + 1, N), dtype=np.uint64)
    glwe[0] = x << np.uint64(LOG_N)                                  # shr_round(., log2 N) gives x back
    ak, rows = const_key((LOG_N, P.k, P.tr_count, P.k + 1), (rnd, 0, lvl0, p0), cls.c, cls.scale_log2)
    return TraceCase(f"{cls.name}@round{rnd}-level{lvl0}-poly{p0}", cls, rnd, at, glwe, ak, rows)


def trace_cases() -> list:
    """four placements (round, (level, poly)) for every whole-polynomial class: each of the first and last round executed, the
    highest reachable and the lowest level, mask and body polynomial occurs twice, and the last round meets level 2 in the body.
    All eight placements are cycled through the one-outlier classes."""
    hi, lo = TRACE_LEVELS
    first, last = TRACE_ROUNDS
    whole = [(first, (hi, 0)), (first, (lo, 1)), (last, (lo, 0)), (last, (hi, 1))]
    where = [(rnd, (lvl, p0)) for rnd in TRACE_ROUNDS for lvl in TRACE_LEVELS for p0 in (0, 1)]
    out = []
    i = 0
    for cls in TRACE_CLASSES:
        if cls.outlier < 0:
            out += [trace_case(cls, rnd, at) for rnd, at in whole]
        else:
            out.append(trace_case(cls, *where[i % len(where)]))
            i += 1
    return out


# ----------------------------------------------------------------------------------------------- blind rotation (2 x 16 bits)

PBS_CLASSES = classes(1 << 15)
PBS_EDGE_CLASSES = ("mixed", "quirk_lookalike", "one_outlier(0)", "one_outlier(1023)", f"one_outlier({128 * 9 + 37})")


def pbs_vector(cls: Cls):
    """(lwe, lut) for `_const_key_engine(cls.c)` (n = 1; row b, level 0, polynomial b): a~ = N makes the decomposed difference
    -2 lut, so a body of -digit * 2^47 puts `digit` into the top digit of every coefficient"""
    lut = np.zeros((P.k + 1, N), dtype=np.uint64)
    lut[P.k] = np.array([(-int(d) << 47) & M64 for d in cls.digits], dtype=np.uint64)
    diff = np.uint64(0) - (lut[P.k] << np.uint64(1))
    assert np.array_equal(digits_array(diff, P.pbs_radix_log, P.pbs_count)[:, 1], cls.d)
    return np.array([1 << 63, 0], dtype=np.uint64), lut.reshape(-1)


# ----------------------------------------------------------------------------------------------- classification

TWO64 = 1 << 64


def classify(vals) -> dict:
    """per value: band ('zero', 'sub52', 'mid' = [2^52, 2^64), 'window' = [2^64, 2^116), 'above'), exponent field, sign,
    quirk (v < 0 and v = 2^63 mod 2^64: `as i64` saturates) and superset (the high word of |v| mod 2^64 is 0x80000000:
    `torus_bits16`'s detector fires), all on Python integers"""
    v = np.asarray(vals, dtype=np.float64).reshape(-1)
    assert np.array_equal(v, np.rint(v)), "the oracle hands rounded values to the conversion"
    ints = [int(x) for x in v]
    mag = np.abs(v)
    band = np.select([mag == 0, mag < 2.0 ** 52, mag < 2.0 ** 64, mag < 2.0 ** 116], ["zero", "sub52", "mid", "window"], "above")
    expo = ((v.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    low = np.array([abs(x) % TWO64 for x in ints], dtype=np.uint64)
    quirk = np.array([x < 0 and x % TWO64 == 1 << 63 for x in ints])
    return dict(band=band, expo=expo, neg=v < 0, quirk=quirk, superset=(low >> np.uint64(32)) == np.uint64(0x80000000), ints=ints)


def rust_conversion(ints) -> np.ndarray:
    """the words `vector_mod_pow2_q_f64` + `as i64` give for integer-valued inputs: v mod 2^64 centred, the residue 2^63 kept
    as +2^63 when it is reached from v < 0 (it then saturates to 0x7FFF...F) and as -2^63 otherwise"""
    out = []
    for x in ints:
        m = abs(x) % TWO64 * (-1 if x < 0 else 1)          # fmod keeps the sign of the dividend
        if m >= 1 << 63:
            m -= TWO64
        elif m <= -(1 << 63):
            m += TWO64
        out.append(min(m, (1 << 63) - 1) & M64)
    return np.array(out, dtype=np.uint64)
