"""Shapes, inputs and bounds shared by tests/test_polynomial_reference.py (oracle against tests/poly_ref.py, CPU) and
tests/test_gpu_polynomial_reference.py (HIP kernels against both).  Test infrastructure; may import the oracle, only to
bring integer key rows into the transform domain (key preparation) and for its parameter record.

A tier-A case is one key (uniform or shaped time-domain rows, NOT an encryption of anything) and a few input items; a
structural deviation (level order, row, sign, rotation) then moves every output word by a uniform amount, distance ~ 1/4.
Where the bounds come from is written in profiles/r07_fft_error.md (the rotation by an encrypted shift, the forward transform
and the packed operations: profiles/r14_exact_reference_new_ops.md); the model is
    sigma_model = 2^(beta - 1 - 53) * sqrt(T * N)     of the torus,
T digit x key polynomial products of radix 2^beta summed into one output polynomial.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import oracle as O
from tests import poly_ref as R
from tests.decomp_ref import M64, recompose

D128 = O.DEFAULT_128
# the generic family's shapes (tests/test_gpu_generic.py) and N = 2048 with another PBS radix
N16 = D128.replace(lwe_n=1, N=16, k=1, pbs_radix_log=6, pbs_count=2, cbs_radix_log=5, cbs_count=3, tr_radix_log=6, tr_count=5,
                   ss_radix_log=5, ss_count=6)
N128K2 = D128.replace(lwe_n=1, N=128, k=2, pbs_radix_log=4, pbs_count=3, cbs_radix_log=4, cbs_count=3)
N256K3 = D128.replace(lwe_n=1, N=256, k=3, pbs_radix_log=4, pbs_count=3, cbs_radix_log=8, cbs_count=2, tr_radix_log=5, tr_count=7,
                      ss_radix_log=4, ss_count=8)
N1024 = D128.replace(lwe_n=1, N=1024, k=1, pbs_radix_log=8, pbs_count=3, cbs_radix_log=4, cbs_count=4)
N2048R = D128.replace(lwe_n=1, pbs_radix_log=8, pbs_count=3)
PBS_SHAPES = {"default128": D128.replace(lwe_n=1), "N16": N16, "N128k2": N128K2, "N256k3": N256K3, "N1024": N1024,
              "N2048_3x8": N2048R}
CMUX_SHAPES = {"default128_4x4": D128, "N16_3x5": N16, "N128k2_3x4": N128K2, "N256k3_2x8": N256K3, "N1024_4x4": N1024}
SS_SHAPES = {"default128_15x3": D128, "N128k2_15x3": N128K2, "N256k3_8x4": N256K3}
CLASSES = ("uniform", "extreme", "one_bin", "small")


def sigma_model(beta: int, terms: int, n: int) -> float:
    return 2.0 ** (beta - 1 - 53) * np.sqrt(terms * n)


def key_fft(rows) -> np.ndarray:
    """integer key rows (..., N) through the oracle's forward transform: the form in which keys reach oracle and library"""
    rows = np.asarray(rows, dtype=np.uint64)
    n = rows.shape[-1]
    return np.stack([O.poly_fft(p) for p in rows.reshape(-1, n)]).reshape(-1)


def cos_poly(n: int, m: int, amp: int) -> np.ndarray:
    """round(amp * cos(pi (2m+1) j / N)): all its energy in transform bin m and its mirror, N/2 times the typical magnitude"""
    ld = np.longdouble
    j = np.arange(n).astype(ld)
    pi = ld("3.14159265358979323846264338327950288")
    return np.rint(ld(amp) * np.cos(pi * ld(2 * m + 1) * j / ld(n))).astype(np.int64).view(np.uint64)


def extreme_word(radix_log: int, count: int, low: bool) -> int:
    d = -(1 << (radix_log - 1)) if low else (1 << (radix_log - 1)) - 1
    return recompose([d] * count, radix_log)


def _key_variants(cls: str, shape, n: int, rng):
    """[(label, rows)] for a key of `shape` + (N,)"""
    full = shape + (n,)
    if cls == "uniform":
        return [("", rng.integers(0, 1 << 64, full, dtype=np.uint64))]
    if cls == "small":
        return [("", rng.integers(0, 1 << 20, full, dtype=np.uint64))]
    if cls == "extreme":
        alt = np.where(np.arange(n) % 2 == 0, np.uint64(1 << 63), np.uint64((1 << 63) - 1))
        return [("key2^63", np.full(full, 1 << 63, dtype=np.uint64)), ("key2^64-1", np.full(full, M64, dtype=np.uint64)),
                ("keyalt", np.broadcast_to(alt, full).copy())]
    out = []
    for m in (0, 3, n // 2 - 1):
        out.append((f"bin{m}", np.broadcast_to(cos_poly(n, m, (1 << 63) - 1), full).copy()))
    return out


def _shaped_polys(cls: str, label: str, radix_log: int, count: int, shape, n: int, rng):
    """the list of GLWE-side word arrays (shape + (N,)) whose digits are decomposed, for a class / key variant"""
    full = shape + (n,)
    if cls in ("uniform", "small"):
        return [rng.integers(0, 1 << 64, full, dtype=np.uint64) for _ in range(2)]
    if cls == "extreme":
        return [np.full(full, extreme_word(radix_log, count, low), dtype=np.uint64) for low in (True, False)]
    m = int(label[3:])
    return [np.broadcast_to(cos_poly(n, m, (1 << 63) - 1), full).copy()]


@dataclass
class Case:
    name: str
    cls: str
    P: object
    key: np.ndarray                 # time-domain rows
    items: list = field(default_factory=list)
    sigma: float = 0.0


# ----------------------------------------------------------------------------------------------- tier A: one-step PBS


def pbs_cases(shape: str, cls: str):
    """one blind-rotation step (lwe_n = 1).  Item = (lwe, lut (k+1, N), log_chi, log_v, body_rotate).  For the shaped classes the
    rotation is a~ = N (mask word 2^63), so the decomposed difference X^N acc - acc is -2 acc, and b~ = 0 through a body word that
    cancels the rotation argument: acc = lut, and lut = -w/2 puts the wanted word w into every decomposed coefficient."""
    P = PBS_SHAPES[shape]
    n, k, lb, cnt = P.N, P.k, P.pbs_radix_log, P.pbs_count
    rng = np.random.default_rng([0xA1, n, k, lb, CLASSES.index(cls)])
    out = []
    for label, key in _key_variants(cls, (k + 1, cnt, k + 1), n, rng):
        c = Case(f"pbs-{shape}-{cls}{'-' + label if label else ''}", cls, P, key[None], sigma=sigma_model(lb, (k + 1) * cnt, n))
        for i, w in enumerate(_shaped_polys(cls, label, lb, cnt, (k + 1,), n, rng)):
            for log_v in (0, 2):
                rot = int(rng.integers(0, 1 << 64, dtype=np.uint64))
                if cls == "uniform":
                    lwe = rng.integers(0, 1 << 64, 2, dtype=np.uint64)
                    lut = w
                elif cls == "small":
                    lwe = rng.integers(0, 1 << 64, 2, dtype=np.uint64)
                    lut = np.zeros_like(w)                                   # sparse LUT: eight full-size coefficients a polynomial
                    idx = rng.integers(0, n, 8)
                    lut[:, idx] = w[:, idx]
                else:
                    lwe = np.array([1 << 63, (-rot) & M64], dtype=np.uint64)
                    lut = np.uint64(0) - (w >> np.uint64(1))                 # w is even: -2 lut = w
                c.items.append((lwe, lut, 0, log_v, rot))
        out.append(c)
    return out


def pbs_exact(c: Case, item, be=R.EXACT):
    lwe, lut, log_chi, log_v, rot = item
    return R.generalized_pbs(lwe, lut, c.key, c.P.pbs_radix_log, c.P.pbs_count, log_chi, log_v, rot, be)


def pbs_oracle(c: Case, item, bsk_fft):
    lwe, lut, log_chi, log_v, rot = item
    x = lwe.copy()
    x[-1:] += np.uint64(rot)
    return O.generalized_pbs(x, lut.reshape(-1), bsk_fft, c.P, log_chi, log_v).reshape(lut.shape)


# ----------------------------------------------------------------------------------------------- tier A: CMUX family


def cmux_cases(shape: str, cls: str):
    """Item = (d0, d1) GLWEs (k+1, N) at the cbs radix; d1 - d0 is the decomposed word array.  The same items serve CMUX,
    multiply_glwe_ggsw (on d1 - d0) and glev_cmux (all items of a case as levels of one GLEV, cycled to cbs_count)."""
    P = CMUX_SHAPES[shape]
    n, k, lb, cnt = P.N, P.k, P.cbs_radix_log, P.cbs_count
    rng = np.random.default_rng([0xA2, n, k, lb, CLASSES.index(cls)])
    out = []
    for label, key in _key_variants(cls, (k + 1, cnt, k + 1), n, rng):
        c = Case(f"cmux-{shape}-{cls}{'-' + label if label else ''}", cls, P, key, sigma=sigma_model(lb, (k + 1) * cnt, n))
        for w in _shaped_polys(cls, label, lb, cnt, (k + 1,), n, rng):
            d0 = rng.integers(0, 1 << 64, (k + 1, n), dtype=np.uint64)
            c.items.append((d0, d0 + w))
        out.append(c)
    return out


def glev_of(c: Case):
    """the case's items cycled into two GLEVs (cbs_count, k+1, N)"""
    cnt = c.P.cbs_count
    a = np.stack([c.items[i % len(c.items)][0] for i in range(cnt)])
    b = np.stack([c.items[i % len(c.items)][1] for i in range(cnt)])
    return a, b


# ----------------------------------------------------------------------------------------------- tier A: rotate-fused CMUX

ROT_SEED = 0        # last word of the rng seed of rot_cases; chosen for the oracle's |z| <= 3 in the uniform case, see the note


def rot_cases(cls: str):
    """one step of the rotation by an encrypted shift at DEFAULT_128, cbs radix 4 x 4 (the rotate-fused kernels' only shape).
    Item = (acc (k+1, N), r): the step is cmux(acc, X^-r acc, key); uniform accumulators go through r = 1, 2, 64 and N/2.
    The decomposed words are X^-r acc - acc and cannot be chosen freely, and r <= N/2 rules out pbs_cases' X^N; the shaped
    classes use r = N/2 and acc = -(X^(-N/2) + 1) (w >> 1): since
    (X^(-N/2) - 1)(X^(-N/2) + 1) = X^-N - 1 = -2, the decomposed words are 2 (w >> 1), the wanted w up to its lowest bit."""
    P = D128
    n, k, lb, cnt = P.N, P.k, P.cbs_radix_log, P.cbs_count
    rng = np.random.default_rng([0xA4, n, k, lb, CLASSES.index(cls), ROT_SEED])
    out = []
    for label, key in _key_variants(cls, (k + 1, cnt, k + 1), n, rng):
        c = Case(f"rot-default128_4x4-{cls}{'-' + label if label else ''}", cls, P, key, sigma=sigma_model(lb, (k + 1) * cnt, n))
        if cls in ("uniform", "small"):
            accs = rng.integers(0, 1 << 64, (4, k + 1, n), dtype=np.uint64)
            c.items = [(acc, r) for r in (1, 2, 64, n // 2) for acc in accs]    # a launch takes one r: four distinct items each
        else:
            for w in _shaped_polys(cls, label, lb, cnt, (k + 1,), n, rng):
                half = w >> np.uint64(1)
                acc = np.uint64(0) - (R.mul_monomial(half, -(n // 2)) + half)
                assert np.array_equal(R.mul_monomial(acc, -(n // 2)) - acc, half << np.uint64(1))
                c.items.append((acc, n // 2))
        out.append(c)
    return out


def rot_exact(c: Case, item, be=R.EXACT):
    return R.rotate_cmux_step(item[0], item[1], c.key, c.P.cbs_radix_log, c.P.cbs_count, be)


def rot_oracle(c: Case, item, g):
    """the oracle's statement of the step: glwe_mul_xn by 2N - r, then cmux"""
    P, (acc, r) = c.P, item
    high = O.glwe_mul_xn(acc.reshape(-1), 2 * P.N - r, P.N, P.k)
    return O.cmux(acc.reshape(-1), high, g, P.N, P.k, P.cbs_radix_log, P.cbs_count).reshape(acc.shape)


# ----------------------------------------------------------------------------------------------- tier A: scheme switch


def ss_cases(shape: str, cls: str):
    """Item = GLEV (cbs_count, k+1, N); its mask polynomials are the decomposed words (scheme-switch radix).  In the small class
    the bodies are small as well (they enter the transform directly)."""
    P = SS_SHAPES[shape]
    n, k, lb, cnt = P.N, P.k, P.ss_radix_log, P.ss_count
    rng = np.random.default_rng([0xA3, n, k, lb, CLASSES.index(cls)])
    out = []
    for label, key in _key_variants(cls, (k * (k + 1) // 2, cnt, k + 1), n, rng):
        c = Case(f"ss-{shape}-{cls}{'-' + label if label else ''}", cls, P, key, sigma=sigma_model(lb, k * cnt, n) + 2.0 ** -54)
        for w in _shaped_polys(cls, label, lb, cnt, (P.cbs_count, k), n, rng):
            body = rng.integers(0, 1 << (20 if cls == "small" else 64), (P.cbs_count, 1, n), dtype=np.uint64)
            c.items.append(np.concatenate([w, body], axis=1))
        out.append(c)
    return out


def ggsw_bins_to_words(bins, P) -> np.ndarray:
    """the FFT-domain GGSW (any leading shape) back to torus words (k+1, levels, k+1, N) by the long-double inverse"""
    b = np.asarray(bins, dtype=np.complex128).reshape(P.k + 1, P.cbs_count, P.k + 1, P.N // 2)
    return R.inverse_twisted_dft_longdouble(b)


# ----------------------------------------------------------------------------------------------- statistics and conditions


def stats(got, exact):
    d = R.torus_distance(got, exact)
    return float(np.sqrt((d ** 2).mean())), float(d.max())


# Classes "extreme" and "one_bin": caps on rms(code) / rms(numpy pipeline) and on max(code) / max(numpy pipeline), where the model
# does not reach.  2 wherever the CPU measurement (profiles/r07_fft_error.md) gave at most 1.5 for both ratios; the cases measured
# above 1.5 are listed with their figures (rms ratio, max ratio) and get 4.  Why they scatter: see the note.
CAP, CAP_MEASURED_ABOVE_1_5 = 2.0, 4.0
MEASURED_ABOVE_1_5 = {
    "pbs-N16-extreme-key2^63": (1.443, 2.000),
    "pbs-N16-extreme-keyalt": (2.117, 1.750),
    "pbs-N128k2-extreme-key2^63": (1.651, 1.500),
    "pbs-N128k2-one_bin-bin0": (1.928, 1.696),
    "pbs-N128k2-one_bin-bin63": (1.868, 1.615),
    "pbs-N256k3-one_bin-bin3": (1.686, 0.958),
    "cmux-default128_4x4-one_bin-bin3": (1.527, 0.952),
    "rot-default128_4x4-one_bin-bin3": (1.527, 0.952),      # profiles/r14_exact_reference_new_ops.md
    "cmux-N128k2_3x4-extreme-key2^63": (1.627, 1.500),
    "cmux-N128k2_3x4-one_bin-bin0": (1.928, 1.696),
    "cmux-N128k2_3x4-one_bin-bin63": (1.868, 1.615),
    "cmux-N1024_4x4-extreme-keyalt": (1.902, 2.173),
    "ss-N128k2_15x3-extreme-key2^64-1": (1.212, 1.663),
    "ss-N256k3_8x4-extreme-key2^64-1": (1.344, 1.764),
    "ss-N256k3_8x4-one_bin-bin3": (2.868, 2.315),
    "ss-N256k3_8x4-one_bin-bin127": (2.640, 1.626),
}


def _distinct(got_list, exact_list, numpy_list):
    """the words of a case as columns (got, exact, numpy), every distinct triple once: a batch repeats its items, and glev_cmux
    repeats the CMUX's own ciphertexts; a repeated word is not a new sample"""
    cat = lambda xs: np.concatenate([np.asarray(x).reshape(-1) for x in xs])  # noqa: E731
    t = np.unique(np.stack([cat(got_list), cat(exact_list), cat(numpy_list)], axis=1), axis=0)
    return t[:, 0], t[:, 1], t[:, 2]


def check_tier_a(c: Case, got_list, exact_list, numpy_list, who: str):
    """the conditions of a tier-A case over all its distinct words together"""
    got, exact, nump = _distinct(got_list, exact_list, numpy_list)
    rms, mx = stats(got, exact)
    nrms, nmx = stats(nump, exact)
    z = R.signed_difference(got, exact).mean() / (rms / np.sqrt(got.size)) if rms else 0.0
    print(f"{c.name:44s} {who:6s} sigma 2^{np.log2(c.sigma):7.2f}  rms {rms / c.sigma:8.3f} max {mx / c.sigma:8.3f}  "
          f"numpy rms {nrms / c.sigma:8.3f} max {nmx / c.sigma:8.3f}  ratio {rms / nrms if nrms else float('nan'):6.3f} "
          f"/ {mx / nmx if nmx else float('nan'):6.3f}  mean/(rms/sqrt n) {z:6.2f}")
    if c.cls == "small":
        assert mx == 0.0, (c.name, who, mx)
    elif c.cls == "uniform":
        assert 0.0 < rms <= 2.0 ** 2.5 * c.sigma, (c.name, who, rms / c.sigma)
        assert mx <= 2.0 ** 5.5 * c.sigma, (c.name, who, mx / c.sigma)
        assert rms <= 2.0 * nrms, (c.name, who, rms / nrms)
        # derived, no measurement: independent roundings have no sign; truncation where the reference rounds would show here
        assert abs(z) <= 6.0, (c.name, who, z)
    else:
        cap = CAP_MEASURED_ABOVE_1_5 if c.name in MEASURED_ABOVE_1_5 else CAP
        assert rms <= cap * nrms, (c.name, who, rms, nrms)
        assert mx <= cap * nmx, (c.name, who, mx, nmx)


def check_scheme_switch(c: Case, got_words, ex, nf, who: str):
    """rows j < k carry the key products; row k is the input GLEV through the forward transform alone, whose 64-bit words do not
    fit an f64: in the small class it is held to the uniform class's conditions instead of to zero"""
    k = c.P.k
    check_tier_a(c, [g[:k] for g in got_words], [e[:k] for e in ex], [f[:k] for f in nf], who)
    row = Case(c.name + "-rowk", "uniform" if c.cls == "small" else c.cls, c.P, None, sigma=c.sigma)
    check_tier_a(row, [g[k] for g in got_words], [e[k] for e in ex], [f[k] for f in nf], who)


def cbs_cmux_phases(hk, lwe, d, ggsw_words_of):
    """exact chain, numpy chain and the chain under test (circuit bootstrap of `lwe`, its GGSW driving one EXACT cmux of the two
    honest GLWEs d): the three phase polynomials"""
    P = hk.P
    out = []
    for g in (R.circuit_bootstrap(lwe, hk.bsk, hk.ak, hk.ssk, P), R.circuit_bootstrap(lwe, hk.bsk, hk.ak, hk.ssk, P, R.NUMPY),
              ggsw_words_of(lwe)):
        out.append(R.glwe_phase(R.cmux(d[0], d[1], g, P.cbs_radix_log, P.cbs_count), hk.glwe_sk))
    return out


def check_tier_b(name: str, got_phase, exact_phase, numpy_phase, who: str, mean_test=True):
    """phase distance to the exact chain against the numpy chain's own, and the bias condition |mean| <= 6 rms / sqrt(count)"""
    rms, mx = stats(got_phase, exact_phase)
    nrms, nmx = stats(numpy_phase, exact_phase)
    sd = R.signed_difference(got_phase, exact_phase)
    mean, count = float(sd.mean()), sd.size
    nmean = float(R.signed_difference(numpy_phase, exact_phase).mean())
    print(f"{name:44s} {who:6s} phase rms 2^{np.log2(rms):7.2f} max 2^{np.log2(mx):7.2f}  numpy rms 2^{np.log2(nrms):7.2f} "
          f"max 2^{np.log2(nmx):7.2f}  ratio {rms / nrms:6.3f}/{mx / nmx:6.3f}  mean/(rms/sqrt n) {mean / (rms / np.sqrt(count)):6.2f} "
          f"(numpy {nmean / (nrms / np.sqrt(count)):6.2f})")
    assert rms <= 2.0 * nrms, (name, who, rms / nrms)
    assert mx <= 2.0 * nmx, (name, who, mx / nmx)
    if mean_test:
        assert abs(mean) <= 6.0 * rms / np.sqrt(count), (name, who, mean, rms, count)
    return dict(case=name, who=who, rms=rms, max=mx, numpy_rms=nrms, numpy_max=nmx, mean=mean, count=count)


# ----------------------------------------------------------------------------------------------- tier B: honest keys

NOISE = 1 << 14      # |e| of every key row: the size of DEFAULT_128's GLWE noise (7e-16 * 2^64 ~ 2^13.6)


@dataclass
class HonestKeys:
    P: object
    lwe_sk: np.ndarray
    glwe_sk: np.ndarray
    bsk: np.ndarray = None
    ak: np.ndarray = None
    ssk: np.ndarray = None


def honest_keys(P, seed: int, bsk=False, ak=False, ssk=False) -> HonestKeys:
    rng = np.random.default_rng([0xB0, seed, P.N, P.k, P.lwe_n])
    hk = HonestKeys(P, R.binary_key(rng, P.lwe_n), R.binary_key(rng, P.k * P.N))
    if bsk:
        hk.bsk = R.bootstrap_key(rng, hk.lwe_sk, hk.glwe_sk, P.N, P.k, P.pbs_radix_log, P.pbs_count, NOISE)
    if ak:
        hk.ak = R.automorphism_keys(rng, hk.glwe_sk, P.N, P.k, P.tr_radix_log, P.tr_count, NOISE)
    if ssk:
        hk.ssk = R.scheme_switch_key(rng, hk.glwe_sk, P.N, P.k, P.ss_radix_log, P.ss_count, NOISE)
    return hk


TRACE_SHAPES = {"default128_6x7": D128, "N256k3_7x5": N256K3}
ROTATION_SHAPES = {"default128_S64": D128.replace(lwe_n=64), "N128k2_S20": N128K2.replace(lwe_n=20),
                   "default128_S637": D128.replace(lwe_n=637)}
CBS_SHAPE = D128.replace(lwe_n=16)


def honest_glwes(P, hk, seed: int, count: int) -> np.ndarray:
    """`count` honest GLWE encryptions of uniform message polynomials: (count, k+1, N)"""
    rng = np.random.default_rng([0xB1, seed, P.N])
    return R.glwe_encrypt(rng, hk.glwe_sk, rng.integers(0, 1 << 64, (count, P.N), dtype=np.uint64), NOISE)


def rotation_inputs(P, seed: int, count: int):
    """uniform LWE words and a uniform random LUT GLWE for each"""
    rng = np.random.default_rng([0xB2, seed, P.N])
    return (rng.integers(0, 1 << 64, (count, P.lwe_n + 1), dtype=np.uint64),
            rng.integers(0, 1 << 64, (count, P.k + 1, P.N), dtype=np.uint64))


# ----------------------------------------------------------------------------------------------- tier B: rotation by an encrypted shift

# name -> (parameters, n_bits, log_stride, the shifts of the four items, seed of keys / inputs / selectors).  The second shape is
# the table lookup's (16 entries of stride 8) and the other ping-pong parity.  Seeds: the oracle's |z| <= 3, see the note.
ENC_SHIFT_SHAPES = {"default128_11bit": (D128, 11, 0, (0, 1, 1365, 2047), 7),
                    "default128_4bit_stride8": (D128, 4, 3, (0, 5, 10, 15), 11)}


def bit_ggsws(rng, hk, value: int, n_bits: int) -> np.ndarray:
    """honest GGSWs (cbs radix, time domain) of the bits of `value`, least significant first: (n_bits, k+1, L, k+1, N)"""
    P = hk.P
    const = np.zeros(P.N, dtype=np.uint64)
    out = []
    for i in range(n_bits):
        const[0] = (value >> i) & 1
        out.append(R.ggsw_encrypt(rng, hk.glwe_sk, const, P.N, P.k, P.cbs_radix_log, P.cbs_count, NOISE))
    return np.stack(out)


@dataclass
class EncShiftCase:
    name: str
    P: object
    n_bits: int
    log_stride: int
    shifts: tuple
    hk: HonestKeys
    glwe: np.ndarray                # (items, k+1, N)
    sel: np.ndarray                 # (items, n_bits, k+1, L, k+1, N), time domain
    exact: np.ndarray = None        # phases of the exact chain and of the numpy chain, (items, N)
    numpy: np.ndarray = None
    steps: list = None              # for every item: [(exact accumulator before step j, r_j)], and the exact result last, (acc, None)


_ENC_SHIFT = {}


def enc_shift_case(shape: str) -> EncShiftCase:
    """the case of a shape with both chains run, built once in a process; the functional condition is asserted on the exact
    chain here: its phase is the input's times X^-(s << log_stride) within 2^-8 of the torus (the gadget's 16 bits over up to 11
    steps, a property of the scheme: measured 2^-9.2 at worst)"""
    if shape not in _ENC_SHIFT:
        P, n_bits, log_stride, shifts, seed = ENC_SHIFT_SHAPES[shape]
        hk = honest_keys(P, seed)
        rng = np.random.default_rng([0xB3, seed, P.N, n_bits])
        c = EncShiftCase(f"encshift-{shape}", P, n_bits, log_stride, shifts, hk, honest_glwes(P, hk, seed, len(shifts)),
                         np.stack([bit_ggsws(rng, hk, s, n_bits) for s in shifts]))
        c.steps = [[] for _ in shifts]
        chain = lambda be, steps: R.glwe_phase(np.stack([R.blind_rotation_by_shift(  # noqa: E731
            c.glwe[i], c.sel[i], log_stride, P.cbs_radix_log, P.cbs_count, be, steps and steps[i]) for i in range(len(shifts))]), hk.glwe_sk)
        c.exact, c.numpy = chain(R.EXACT, c.steps), chain(R.NUMPY, None)
        for i, st in enumerate(c.steps):
            st.append((R.blind_rotation_by_shift(st[-1][0], c.sel[i][-1:], st[-1][1].bit_length() - 1, P.cbs_radix_log, P.cbs_count), None))
        check_rotated_phase(c, c.exact, "exact")
        _ENC_SHIFT[shape] = c
    return _ENC_SHIFT[shape]


def enc_shift_oracle(c: EncShiftCase, i: int, sel_fft, glwe=None) -> np.ndarray:
    """the oracle's loop for item i (or for `glwe` under item i's selectors): glwe_mul_xn by 2N - 2^(step + log_stride), then
    cmux, steps ascending; sel_fft (n_bits, bins)"""
    P = c.P
    acc = (c.glwe[i] if glwe is None else glwe).reshape(-1)
    for step in range(c.n_bits):
        high = O.glwe_mul_xn(acc, 2 * P.N - (1 << (step + c.log_stride)), P.N, P.k)
        acc = O.cmux(acc, high, sel_fft[step], P.N, P.k, P.cbs_radix_log, P.cbs_count)
    return acc.reshape(P.k + 1, P.N)


def check_step_bias(c: EncShiftCase, step, who: str):
    """The bias of the chain, asserted on WORDS as tests/test_polynomial_reference.py's rotation_case does: every step restarted
    from the exact accumulator by `step(item, j, acc, r)`, its signed word error against the exact next accumulator pooled over all
    steps of all items.  Word errors of a step are independent roundings; a bias of b a step would grow to n_bits b over the chain.
    (The phases' own mean is no such statistic: every mask error enters every phase coefficient through the same key.)"""
    d = []
    for i, st in enumerate(c.steps):
        for j in range(c.n_bits):
            d.append(R.signed_difference(step(i, j, st[j][0], st[j][1]), st[j + 1][0]))
    d = np.concatenate(d, axis=None)
    z = d.mean() / (d.std() / np.sqrt(d.size))
    print(f"{c.name:44s} {who:6s} per-step word bias over {d.size} words: rms 2^{np.log2(d.std()):.2f}  mean/(rms/sqrt n) {z:6.2f}")
    assert 0.0 < d.std() <= 2.0 ** 2.5 * sigma_model(c.P.cbs_radix_log, (c.P.k + 1) * c.P.cbs_count, c.P.N), (c.name, who, d.std())
    assert abs(z) <= 6.0, (c.name, who, z)


def check_rotated_phase(c: EncShiftCase, phase, who: str):
    """the chain means what it should: phase_in * X^-(s << log_stride), within 2^-8"""
    want = np.stack([R.mul_monomial(R.glwe_phase(c.glwe[i], c.hk.glwe_sk), -(s << c.log_stride)) for i, s in enumerate(c.shifts)])
    d = float(R.torus_distance(phase, want).max())
    print(f"{c.name:44s} {who:6s} distance to the rotated input phase: max 2^{np.log2(d):.2f}")
    assert d <= 2.0 ** -8, (c.name, who, d)


# ----------------------------------------------------------------------------------------------- the forward transform

FFT_SIZES = (2048, 256, 16)


def fft_cases(n: int):
    """[(name, polynomials (P, N) uint64)] for the forward transform alone.  A delta has a single twiddle in every bin: it reads
    the tables directly."""
    rng = np.random.default_rng([0xA5, n])
    delta = np.zeros((8, n), dtype=np.uint64)
    at = (0, 1, 3, n // 3, n // 2 - 1, n // 2, n // 2 + 1, n - 1)
    assert len(set(at)) == 8
    delta[np.arange(8), at] = 1 << 62
    return [(f"fft-N{n}-uniform", rng.integers(0, 1 << 64, (8, n), dtype=np.uint64)),
            (f"fft-N{n}-small", rng.integers(0, 1 << 20, (3, n), dtype=np.uint64)),
            (f"fft-N{n}-delta", delta),
            (f"fft-N{n}-const2^63", np.full((1, n), 1 << 63, dtype=np.uint64)),
            (f"fft-N{n}-one_bin", np.stack([cos_poly(n, m, (1 << 63) - 1) for m in (0, 3, n // 2 - 1)]))]


@functools.lru_cache(maxsize=None)
def fft_references(n: int):
    """{name: (long-double bins, numpy bins)} of fft_cases(n), computed once in a process"""
    return {name: (R.forward_twisted_dft_longdouble(R.signed(p)), R.NUMPY.forward_bins(R.signed(p))) for name, p in fft_cases(n)}


def forward_error(bins, exact):
    """|X - X_exact| of every bin over the rms bin magnitude of its polynomial: (rms, max) over the case"""
    exact = np.asarray(exact, dtype=np.clongdouble)
    e = np.abs(np.asarray(bins).astype(np.clongdouble) - exact) / np.sqrt((np.abs(exact) ** 2).mean(axis=-1, keepdims=True))
    return float(np.sqrt((e ** 2).mean())), float(e.max())


def check_forward(name: str, bins, exact, numpy_bins, who: str):
    """the transform's error against the long-double DFT, held to the numpy yardstick's on the same inputs: rms <= 2 x, max <= 4 x
    (measured for the oracle: rms ratio <= 1.1, max ratio <= 2.1; the max is one sample's, hence the factor two over it)"""
    rms, mx = forward_error(bins, exact)
    nrms, nmx = forward_error(numpy_bins, exact)
    print(f"{name:44s} {who:6s} rms {rms:9.3e} max {mx:9.3e}  numpy rms {nrms:9.3e} max {nmx:9.3e}  "
          f"ratio {rms / nrms if nrms else float('nan'):6.3f} / {mx / nmx if nmx else float('nan'):6.3f}")
    assert rms <= 2.0 * nrms, (name, who, rms, nrms)
    assert mx <= 4.0 * nmx, (name, who, mx, nmx)
    return rms, mx, nrms, nmx


# ----------------------------------------------------------------------------------------------- the model across shapes


def cmux_model_table():
    """CMUX with uniform inputs, oracle and numpy pipeline against the exact product, at the radices the project uses and the
    generic family's corners: `python -m tests.polyref_cases` prints the table of profiles/r07_fft_error.md"""
    rows = [(2048, 1, 2, 16), (2048, 1, 4, 4), (2048, 1, 6, 7), (2048, 1, 15, 3), (256, 3, 3, 8), (16, 1, 2, 16), (1024, 1, 3, 12)]
    print("| N, k, count x beta | sigma_model | oracle rms / max (in sigma) | numpy rms / max (in sigma) | rms ratio |")
    print("|---|---|---|---|---|")
    for n, k, cnt, lb in rows:
        rng = np.random.default_rng([0xA0, n, k, cnt, lb])
        key = rng.integers(0, 1 << 64, (k + 1, cnt, k + 1, n), dtype=np.uint64)
        d0, d1 = rng.integers(0, 1 << 64, (2, k + 1, n), dtype=np.uint64)
        exact = R.cmux(d0, d1, key, lb, cnt)
        got = O.cmux(d0.reshape(-1), d1.reshape(-1), key_fft(key), n, k, lb, cnt).reshape(k + 1, n)
        sig = sigma_model(lb, (k + 1) * cnt, n)
        (r, m), (nr, nm) = stats(got, exact), stats(R.cmux(d0, d1, key, lb, cnt, R.NUMPY), exact)
        print(f"| {n}, {k}, {cnt} x {lb} | 2^{np.log2(sig):.2f} | {r / sig:.3f} / {m / sig:.2f} | {nr / sig:.3f} / {nm / sig:.2f} | {r / nr:.2f} |")


if __name__ == "__main__":
    cmux_model_table()
