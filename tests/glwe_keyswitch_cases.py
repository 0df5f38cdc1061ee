"""Shapes, keys, inputs and oracle-level references shared by tests/test_glwe_keyswitch_reference.py (CPU: the oracle's three
functions against each other and against decryption) and tests/test_gpu_glwe_keyswitch.py (the HIP kernels against the oracle,
word for word).  Test infrastructure.

The three functions (sunscreen_tfhe/src/ops):
  keyswitch_glwe_to_glwe   fft_ops.rs:457-495          O.keyswitch_glwe_to_glwe
  one automorphism round   polynomial/mod.rs:62-84 + the keyswitch back (automorphisms/mod.rs:72-83)     oracle_round
  trace                    automorphisms/mod.rs:53-85  O.trace
Keys are honest (tests/polyref_cases.py): binary secret keys, |e| <= NOISE in every key row.  A case holds five different honest
GLWEs, so that a wrong item index shows in any batch."""
import functools
from dataclasses import dataclass

import numpy as np

import oracle as O
from tests import poly_ref as R
from tests import polyref_cases as C

U = np.uint64
# the hand-written kernel's shape, a k = 3 shape whose keyswitch walks the row loop, and the smallest degree
SHAPES = dict(C.TRACE_SHAPES, N16=C.N16)
ITEMS = 5
PLAIN_BITS = 12                       # the reference's own `can_trace` (ops/automorphisms/mod.rs:101-136)
OTHER_RADIX = (8, 4)                  # (radix_log, radix_count) of the key a DEFAULT_128 context must hand to the generic kernel


def log2n(P) -> int:
    return P.N.bit_length() - 1


def exponents(P) -> list:
    """t_round = N / 2^(round - 1) + 1 for round = 1 .. log2 N (ops/automorphisms/mod.rs:35-36, 72-73)"""
    return R.trace_exponents(P.N)


@dataclass
class KsCase:
    name: str
    P: object
    hk: object                # honest keys with the automorphism keys, (log2 N, k, L, k+1, N) words
    ak_fft: np.ndarray        # (log2 N, bins of one keyswitch key)
    sk_b: np.ndarray          # the second secret key
    ksk: np.ndarray           # sk_a -> sk_b at the trace radix, (k, L, k+1, N) words
    ksk_fft: np.ndarray
    x: np.ndarray             # (ITEMS, k+1, N) honest GLWEs under sk_a


@functools.lru_cache(maxsize=None)
def case(shape: str) -> KsCase:
    P = SHAPES[shape]
    hk = C.honest_keys(P, 32, ak=True)
    rng = np.random.default_rng([0xC7, P.N, P.k])
    sk_b = R.binary_key(rng, P.k * P.N)
    ksk = R.glwe_keyswitch_key(rng, hk.glwe_sk, sk_b, P.N, P.k, P.tr_radix_log, P.tr_count, C.NOISE)
    x = C.honest_glwes(P, hk, 32, ITEMS)
    c = KsCase(shape, P, hk, C.key_fft(hk.ak).reshape(log2n(P), -1), sk_b, ksk, C.key_fft(ksk), x)
    for a in (c.ak_fft, c.ksk, c.ksk_fft, c.x, hk.ak):
        a.setflags(write=False)
    return c


def other_radix_key(c: KsCase, seed: int = 1):
    """sk_a -> sk_b at OTHER_RADIX: (words (k, L, k+1, N), spectra)"""
    lg, cnt = OTHER_RADIX
    rng = np.random.default_rng([0xC8, c.P.N, seed])
    ksk = R.glwe_keyswitch_key(rng, c.hk.glwe_sk, c.sk_b, c.P.N, c.P.k, lg, cnt, C.NOISE)
    return ksk, C.key_fft(ksk)


def second_key(c: KsCase):
    """another sk_a -> sk_b key at the trace radix (other masks, other noise): what a reload must switch to"""
    rng = np.random.default_rng([0xC9, c.P.N])
    ksk = R.glwe_keyswitch_key(rng, c.hk.glwe_sk, c.sk_b, c.P.N, c.P.k, c.P.tr_radix_log, c.P.tr_count, C.NOISE)
    return ksk, C.key_fft(ksk)


# ---- the oracle's statements --------------------------------------------------------------------------------------------------

def oracle_keyswitch(P, x, ksk_fft, radix=None) -> np.ndarray:
    """O.keyswitch_glwe_to_glwe on one GLWE (k+1, N) or on a batch"""
    lg, cnt = radix or (P.tr_radix_log, P.tr_count)
    x = np.asarray(x, dtype=U)
    if x.ndim == 3:
        return np.stack([oracle_keyswitch(P, g, ksk_fft, radix) for g in x])
    return O.keyswitch_glwe_to_glwe(x.reshape(-1), ksk_fft, P.N, P.k, lg, cnt).reshape(P.k + 1, P.N)


def oracle_pow_k(P, x, t: int) -> np.ndarray:
    """`polynomial_pow_k` on every polynomial of a GLWE (k+1, N)"""
    return np.stack([O.poly_pow_k(p, t) for p in np.asarray(x, dtype=U)])


def oracle_round(c: KsCase, x, rnd: int) -> np.ndarray:
    """round `rnd` in 1 .. log2 N of the trace's loop, without the add: keyswitch(x(X^t), ak[rnd - 1])"""
    x = np.asarray(x, dtype=U)
    if x.ndim == 3:
        return np.stack([oracle_round(c, g, rnd) for g in x])
    return oracle_keyswitch(c.P, oracle_pow_k(c.P, x, exponents(c.P)[rnd - 1]), c.ak_fft[rnd - 1])


def oracle_fold(c: KsCase, x) -> np.ndarray:
    """x <- x + round(x) over the rounds in turn: what `trace` is made of"""
    x = np.asarray(x, dtype=U).copy()
    for rnd in range(1, log2n(c.P) + 1):
        x = x + oracle_round(c, x, rnd)
    return x


@functools.lru_cache(maxsize=None)
def oracle_traces(shape: str) -> np.ndarray:
    """O.trace of every item of the case, computed once in a process: (ITEMS, k+1, N)"""
    c = case(shape)
    out = np.stack([O.trace(g.reshape(-1), c.ak_fft.reshape(-1), c.P).reshape(c.P.k + 1, c.P.N) for g in c.x])
    out.setflags(write=False)
    return out


def cbs_levels(P, glwe) -> np.ndarray:
    """what `mod_switch_trace_and_rotate` hands to its trace for a lo-noise GLWE (k+1, N), in exact integers (tests/poly_ref.py's
    statement of circuit_bootstrapping.rs:260-298): level i = shr_round(X^-i * (glwe + sum_{l <= i} 2^(64 - logB (l+1) - 1) X^l),
    log2 N), the half units accumulating from level to level: (cbs_count, k+1, N)"""
    rotated = np.asarray(glwe, dtype=U).copy()
    staged = []
    for i in range(P.cbs_count):
        rotated[P.k, i] += U(1 << (64 - P.cbs_radix_log * (i + 1) - 1))
        staged.append(R.shr_round(R.mul_monomial(rotated, -i), log2n(P)))
    return np.stack(staged)


# ---- `can_trace` -------------------------------------------------------------------------------------------------------------

def all_ones_glwe(c: KsCase) -> np.ndarray:
    """an honest encryption of the polynomial whose every coefficient is 1 at PLAIN_BITS plaintext bits: (k+1, N)"""
    rng = np.random.default_rng([0xCA, c.P.N])
    msg = np.full((1, c.P.N), 1 << (64 - PLAIN_BITS), dtype=U)
    return R.glwe_encrypt(rng, c.hk.glwe_sk, msg, C.NOISE)[0]


def decode(phase) -> np.ndarray:
    """the reference's decode at PLAIN_BITS: round to the nearest multiple of 2^(64 - PLAIN_BITS), mod 2^PLAIN_BITS"""
    p = np.asarray(phase, dtype=U)
    sh = U(64 - PLAIN_BITS)
    return ((p >> sh) + ((p >> (sh - U(1))) & U(1))) & U((1 << PLAIN_BITS) - 1)


def check_can_trace(c: KsCase, traced, who: str):
    """N in coefficient 0 and 0 elsewhere (ops/automorphisms/mod.rs:129-135)"""
    got = decode(R.glwe_phase(np.asarray(traced, dtype=U).reshape(c.P.k + 1, c.P.N), c.hk.glwe_sk))
    want = np.zeros(c.P.N, dtype=U)
    want[0] = c.P.N % (1 << PLAIN_BITS)
    assert np.array_equal(got, want), (c.name, who, np.argwhere(got != want)[:8].ravel(), got[:4])


# the decode radius at PLAIN_BITS, of the torus: a phase error below it leaves every 12-bit message in place.  It is the
# reference's decode, not a figure of the code under test (measured: 4.5e-11 at DEFAULT_128, 7.4e-10 at N256k3_7x5).
DECODE_RADIUS = 2.0 ** -(PLAIN_BITS + 1)


def check_switched_phase(c: KsCase, x, switched, who: str) -> float:
    """the phase of `switched` under sk_b is the phase of `x` under sk_a, within the decode radius"""
    d = float(R.torus_distance(R.glwe_phase(switched, c.sk_b), R.glwe_phase(x, c.hk.glwe_sk)).max())
    print(f"keyswitch a->b {c.name:16s} {who:8s} phase error max {d:.3e} of the torus (decode radius {DECODE_RADIUS:.3e})")
    assert d < DECODE_RADIUS, (c.name, who, d)
    return d
