"""The gadget decomposition and the LWE keyswitch at every radix the ABI accepts, on the CPU: the independent restatement of
tests/decomp_ref.py against its own algebra, and the oracle against it (the oracle had only been checked at the parameter
sets the GPU tests use).  The GPU side is tests/test_gpu_decompositions.py."""
import numpy as np
import pytest

import oracle as O
from tests.decomp_ref import (M64, digits_array, extreme_words, keyswitch_ref, lwe_phase, noiseless_keyswitch_phase,
                              radix_digits, radix_round, recompose, round_to_grid)

# every (logB, l) the keyswitch accepts (0 < l * logB <= 32), and the generic family's PBS / CBS / trace / scheme-switch
# radices (l * logB < 64)
KS_RADICES = [(lg, c) for lg in range(1, 33) for c in range(1, 32 // lg + 1)]
GENERIC_RADICES = [(lg, c) for lg in range(1, 64) for c in range(1, 63 // lg + 1)]


def _words(lg, c, rng, n=48):
    return extreme_words(lg, c) + [int(x) for x in rng.integers(0, 1 << 64, size=n, dtype=np.uint64)]


@pytest.mark.parametrize("lg", range(1, 64))
def test_digits_lie_in_range_and_recompose_to_the_rounded_word(lg):
    rng = np.random.default_rng(1000 + lg)
    lo, hi = -(1 << (lg - 1)), (1 << (lg - 1)) - 1
    for l_ in [c for g, c in GENERIC_RADICES if g == lg]:
        for x in _words(lg, l_, rng):
            d = radix_digits(x, lg, l_)
            assert len(d) == l_
            assert all(lo <= v <= hi for v in d), (lg, l_, hex(x), d)
            assert recompose(d, lg) == round_to_grid(x, lg, l_), (lg, l_, hex(x))
            # the rounding is to the nearest grid point: at most half a step away, mod 2^64
            step = 1 << (64 - lg * l_)
            err = (x - recompose(d, lg)) & M64
            assert err <= step // 2 or M64 + 1 - err <= step // 2, (lg, l_, hex(x))


@pytest.mark.parametrize("lg", range(1, 64))
def test_digit_vectors_at_the_extremes_decompose_back_to_themselves(lg):
    rng = np.random.default_rng(2000 + lg)
    lo, hi = -(1 << (lg - 1)), (1 << (lg - 1)) - 1
    for l_ in [c for g, c in GENERIC_RADICES if g == lg]:
        cases = [[lo] * l_, [hi] * l_, [0] * l_, [lo if j % 2 else hi for j in range(l_)],
                 [hi if j % 2 else lo for j in range(l_)], [int(v) for v in rng.integers(lo, hi + 1, size=l_)]]
        below = (1 << (63 - lg * l_)) - 1        # anything under half a step rounds away
        for ds in cases:
            w = recompose(ds, lg)
            assert radix_digits(w, lg, l_) == ds, (lg, l_, ds)
            assert radix_digits((w + below) & M64, lg, l_) == ds, (lg, l_, ds)
            assert radix_digits((w - below - 1) & M64, lg, l_) == ds, (lg, l_, ds)


def test_numpy_digits_equal_the_integer_statement():
    rng = np.random.default_rng(3)
    for lg, l_ in GENERIC_RADICES[::7] + [(32, 1), (8, 4), (2, 6), (1, 63), (63, 1), (21, 3), (31, 2)]:
        xs = np.array(_words(lg, l_, rng, 16), dtype=np.uint64)
        got = digits_array(xs, lg, l_)
        for x, row in zip(xs, got):
            assert list(row) == radix_digits(int(x), lg, l_), (lg, l_, hex(int(x)))


@pytest.mark.parametrize("lg", [1, 2, 3, 7, 8, 9, 13, 16, 17, 21, 31, 32, 40, 48, 62, 63])
def test_oracle_decomposition_equals_the_reference(lg):
    rng = np.random.default_rng(4000 + lg)
    for l_ in [c for g, c in GENERIC_RADICES if g == lg]:
        xs = np.array(_words(lg, l_, rng, 25), dtype=np.uint64)
        got = O.decompose_poly(xs, lg, l_)          # [l][N], digit j least significant first, as u64
        want = digits_array(xs, lg, l_).T.copy().view(np.uint64)
        assert np.array_equal(got, want), (lg, l_)
        for x in xs[:12]:
            assert O.radix_round(int(x), lg, l_) == radix_round(int(x), lg, l_), (lg, l_, hex(int(x)))


def _ks_inputs(lg, c, n_in, rng, B=6):
    ext = extreme_words(lg, c)
    rows = [rng.integers(0, 1 << 64, size=n_in + 1, dtype=np.uint64) for _ in range(B)]
    for x in ext:                     # rows of one extreme word, and a row mixing them column by column
        rows.append(np.full(n_in + 1, x, dtype=np.uint64))
    rows.append(np.array([ext[i % len(ext)] for i in range(n_in + 1)], dtype=np.uint64))
    return np.stack(rows)


def _synthetic_keys(n_in, c, w, rng):
    size = n_in * c * w
    alt = np.where(np.arange(size) % 2 == 0, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555).astype(np.uint64)
    mix = np.where(np.arange(size) % 3 == 0, 0, M64).astype(np.uint64)
    return {"random": rng.integers(0, 1 << 64, size=size, dtype=np.uint64), "zero": np.zeros(size, dtype=np.uint64),
            "ones": np.full(size, M64, dtype=np.uint64), "alternating": alt, "00FF": mix}


@pytest.mark.parametrize("lg", range(1, 33))
def test_oracle_keyswitch_equals_the_reference_at_every_radix(lg):
    n_in, n_out = 64, 5
    rng = np.random.default_rng(5000 + lg)
    for c in [c for g, c in KS_RADICES if g == lg]:
        ct = _ks_inputs(lg, c, n_in, rng)
        for name, ksk in _synthetic_keys(n_in, c, n_out + 1, rng).items():
            want = keyswitch_ref(ct, ksk, n_in, n_out, lg, c)
            for i in range(ct.shape[0]):
                assert np.array_equal(O.keyswitch_lwe(ct[i], ksk, n_in, n_out, lg, c), want[i]), (lg, c, name, i)
            assert np.array_equal(keyswitch_ref(ct[0], ksk, n_in, n_out, lg, c), want[0])


def test_keyswitch_reference_by_hand():
    """two input words, one output word: the definition written out"""
    lg, c, n_in, n_out = 4, 2, 2, 0
    ksk = np.array([3, 5, 7, 11], dtype=np.uint64)     # KSK[i][j], one word each
    ct = np.array([0x7F << 56, 0x08 << 56, 100], dtype=np.uint64)
    # least significant digit first: 0x7F = -1 + 16 * -8 (mod 256), 0x08 = -8 + 16 * 1
    assert radix_digits(0x7F << 56, lg, c) == [-1, -8] and radix_digits(0x08 << 56, lg, c) == [-8, 1]
    d0, d1 = radix_digits(0x7F << 56, lg, c), radix_digits(0x08 << 56, lg, c)
    want = (100 - (d0[0] * 5 + d0[1] * 3 + d1[0] * 11 + d1[1] * 7)) & M64
    assert keyswitch_ref(ct, ksk, n_in, n_out, lg, c)[0] == want
    assert O.keyswitch_lwe(ct, ksk, n_in, n_out, lg, c)[0] == want


@pytest.mark.parametrize("lg,c", [(1, 1), (1, 32), (2, 6), (3, 10), (4, 8), (8, 4), (9, 3), (11, 2), (16, 2), (31, 1),
                                  (32, 1)])
def test_noiseless_keyswitch_decrypts_to_the_rounded_phase(lg, c):
    n_in, n_out = 128, 5
    r = O.Rng(0xD3C0 + 64 * lg + c)
    s_in, s_out = O.gen_binary_key(r, n_in), O.gen_binary_key(r, n_out)
    ksk = O.gen_ksk(r, s_in, s_out, lg, c, 0.0)
    rng = np.random.default_rng(6000 + lg)
    ct = _ks_inputs(lg, c, n_in, rng)
    want = noiseless_keyswitch_phase(ct, s_in, lg, c)
    ref = keyswitch_ref(ct, ksk, n_in, n_out, lg, c)
    assert np.array_equal(lwe_phase(ref, s_out), want), (lg, c)
    for i in range(ct.shape[0]):
        out = O.keyswitch_lwe(ct[i], ksk, n_in, n_out, lg, c)
        assert np.array_equal(out, ref[i]), (lg, c, i)
        assert O.decrypt_lwe_raw(out, s_out) == int(want[i]), (lg, c, i)
